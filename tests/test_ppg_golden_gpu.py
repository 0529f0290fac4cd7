"""GPU parity of the whole-episode kernels against the reference's own outputs (tests/golden/ppg_rnn_parts.npz, written
by make_golden_ppg.py from ppg_rnn_lunarlander.py's EpisodeBuffer.compute_advantage and PPGTrainer.update()):
per-episode GAE, and the L5 / L6 losses and gradients including saturated probabilities, the dual clip and its tie."""
import numpy as np
import pytest

from conftest import load_golden, rel_close

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def test_episode_gae_matches_reference(dev):
    from gymrl_amd import ops
    g = load_golden("ppg_rnn_parts")
    td = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    gamma, lam = g["gae_gamma_lam"]
    adv_n, vt, raw = ops.episode_gae(td(g["gae_rew"]), td(g["gae_val"]), td(g["gae_next_val"]),
                                     td(g["gae_done"].astype(np.uint8)), td(g["gae_dw"].astype(np.uint8)), g["gae_offsets"],
                                     gamma, lam, want_raw=True)
    assert np.array_equal(raw.cpu().numpy(), g["gae_adv_raw"])
    assert np.array_equal(vt.cpu().numpy(), g["gae_v_target"])
    got, want = adv_n.cpu().numpy(), g["gae_adv_norm"]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert rel_close(got[ok], want[ok], 1e-6) <= 1e-6


@pytest.mark.parametrize("k", [0, 1, 2])
def test_l5_l6_match_reference_update(dev, k):
    from gymrl_amd import ops
    g = load_golden("ppg_rnn_parts")
    clip, dual, vc, ec, beta = (float(x) for x in g["loss_cfg"])
    c = {n: g[f"l{k}_{n}"] for n in ("logits", "value", "aux", "act", "old_logp", "adv", "v_target")}
    td = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    n = c["value"].size
    offs = [0, n]
    dz, dv, mp = ops.ppg_policy_loss_fwd_bwd(td(c["logits"]), td(c["value"]), td(c["act"]), td(c["old_logp"]),
                                             td(c["adv"]), td(c["v_target"]), offs, clip, dual, vc, ec)
    dza, dva, ma = ops.ppg_aux_loss_fwd_bwd(td(c["logits"]), td(c["aux"]), td(c["act"]), td(c["old_logp"]),
                                            td(c["v_target"]), offs, beta)
    m = g[f"l{k}_metrics"]                                              # total, clip, value, entropy, advantage, aux value
    assert rel_close(mp.cpu().numpy()[0], m[:5]) <= 1e-5
    assert rel_close(ma.cpu().numpy()[0, 0], m[5]) <= 1e-5
    # per-token gradients are O(1 / n): compared at O(1)
    assert rel_close(dz.cpu().numpy() * n, g[f"l{k}_dlogits_policy"] * n) <= 1e-5
    assert rel_close(dv.cpu().numpy() * n, g[f"l{k}_dvalue"] * n) <= 1e-5
    assert rel_close(dza.cpu().numpy() * n, g[f"l{k}_dlogits_aux"] * n) <= 1e-5
    assert rel_close(dva.cpu().numpy() * n, g[f"l{k}_daux"] * n) <= 1e-5
    if k == 0:
        assert not dza.cpu().numpy()[1].any()                            # the clamped log passes no gradient
        # the torch.max tie at ratio == dual_clip: its rows carry half of the surrogate's gradient, bit-close to torch
        assert rel_close(dz.cpu().numpy()[12:16] * n, g["l0_dlogits_policy"][12:16] * n) <= 1e-5

"""GPU checks of the per-episode kernels of the whole-episode recurrent trainers: gymrl_episode_gae against the
reference's compute_advantage arithmetic, and L5 / L6 (gymrl_ppg_policy_loss_fwd_bwd / gymrl_ppg_aux_loss_fwd_bwd)
against torch autograd over Categorical(probs), including saturated probabilities and the dual clip
(the tie of torch.max at ratio == dual_clip is pinned by test_ppg_golden_gpu.py).  The shapes reach every row form
(A = 2 .. 8), the 256-thread block-stride loop with all four waves in block_sum (episodes of 255 .. 600 rows), the second
launch of 255 segments (more than 255 episodes: seg0 != 0 offsets metrics_ep and ep_moments) and the hand-over of the GAE
carry between two 2048-step LDS chunks."""
import numpy as np
import pytest

from conftest import rel_close

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CLIP, DUAL, VC, EC, BETA = 0.2, 3.0, 0.5, 1e-2, 1.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def td(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _compute_advantage(rew, done, dw, val, nv, gamma, lam):
    """EpisodeBuffer.compute_advantage (ppg_rnn_lunarlander.py:198-215), one episode, in its float32 operation order."""
    td_err = (rew + np.float32(gamma) * nv * (np.float32(1) - dw)) - val
    adv, gae = [], np.float32(0)
    for delta, d in zip(td_err[::-1], done[::-1]):
        gae = np.float32(gamma * lam) * gae * (np.float32(1) - d) + delta
        adv.append(gae)
    adv = np.array(adv[::-1], np.float32)
    vt = adv + val
    t = torch.from_numpy(adv)
    return adv, vt, ((t - t.mean()) / (t.std() + 1e-8)).numpy()


def test_episode_gae_matches_compute_advantage(dev):
    from gymrl_amd import ops
    rng = np.random.default_rng(11)
    lens = [1, 9, 21, 1000, 3000, 2, 57]
    offs = np.concatenate([[0], np.cumsum(lens)])
    M = int(offs[-1])
    rew = (rng.normal(size=M) * 3).astype(np.float32)
    val, nv = rng.normal(size=M).astype(np.float32), rng.normal(size=M).astype(np.float32)
    done, dw = np.zeros(M, np.float32), np.zeros(M, np.float32)
    done[offs[1:] - 1] = 1
    dw[offs[1:] - 1] = (rng.random(len(lens)) < 0.5)
    done[offs[3] + 500] = 1                                            # a done inside an episode resets the recursion there
    mom = torch.empty(len(lens), 2, dtype=torch.float64, device=dev)
    adv_n, vt, raw = ops.episode_gae(td(rew, dev), td(val, dev), td(nv, dev), td(done.astype(np.uint8), dev),
                                     td(dw.astype(np.uint8), dev), offs, 0.995, 0.95, want_raw=True, ep_moments=mom)
    adv_n, vt, raw = adv_n.cpu().numpy(), vt.cpu().numpy(), raw.cpu().numpy()
    for e, n in enumerate(lens):
        s = slice(offs[e], offs[e + 1])
        a, v, an = _compute_advantage(rew[s], done[s], dw[s], val[s], nv[s], 0.995, 0.95)
        assert np.array_equal(raw[s], a) and np.array_equal(vt[s], v), e
        if n == 1:
            assert np.isnan(adv_n[s]).all() and np.isnan(an).all()     # torch's unbiased std of one element is NaN
        else:
            assert rel_close(adv_n[s], an) <= 1e-5, e
            assert abs(float(adv_n[s].astype(np.float64).mean())) <= 1e-5
    assert np.allclose(mom.cpu().numpy()[:, 0], [raw[offs[e]:offs[e + 1]].astype(np.float64).mean() for e in range(len(lens))])


def _gae_inputs(rng, lens):
    offs = np.concatenate([[0], np.cumsum(lens)])
    M = int(offs[-1])
    rew = (rng.normal(size=M) * 3).astype(np.float32)
    val, nv = rng.normal(size=M).astype(np.float32), rng.normal(size=M).astype(np.float32)
    done, dw = np.zeros(M, np.float32), np.zeros(M, np.float32)
    done[offs[1:] - 1] = 1
    dw[offs[1:] - 1] = (rng.random(len(lens)) < 0.5)
    return offs, rew, val, nv, done, dw


def _run_episode_gae(dev, offs, rew, val, nv, done, dw, mom):
    from gymrl_amd import ops
    out = ops.episode_gae(td(rew, dev), td(val, dev), td(nv, dev), td(done.astype(np.uint8), dev), td(dw.astype(np.uint8), dev),
                          offs, 0.995, 0.95, want_raw=True, ep_moments=mom)
    return tuple(x.cpu().numpy() for x in out)


def test_episode_gae_chunk_boundaries(dev):
    """Episodes around the 2048-step LDS chunk: one step short of a chunk, exactly one, one more, exactly two, two and one.
    Chunks count back from the episode's end, so the first hand-over of `carry` lies between rows n - 2049 and n - 2048 and
    the second between n - 4097 and n - 4096: an extra done on either side of each (the one on the later row cuts the
    carry that is handed over; the one on the earlier row resets a carry that has just arrived)."""
    rng = np.random.default_rng(12)
    lens = [2047, 2048, 2049, 4096, 4097]
    offs, rew, val, nv, done, dw = _gae_inputs(rng, lens)
    planted = 0
    for e, n in enumerate(lens):
        for pos in (n - 2049, n - 2048, n - 4097, n - 4096):
            if 0 <= pos < n - 1:
                done[offs[e] + pos] = 1
                planted += 1
    assert planted == 1 + 2 + 3 + 4
    mom = torch.full((len(lens), 2), -7.25, dtype=torch.float64, device=dev)
    adv_n, vt, raw = _run_episode_gae(dev, offs, rew, val, nv, done, dw, mom)
    for e in range(len(lens)):
        s = slice(offs[e], offs[e + 1])
        a, v, an = _compute_advantage(rew[s], done[s], dw[s], val[s], nv[s], 0.995, 0.95)
        assert np.array_equal(raw[s], a) and np.array_equal(vt[s], v), e
        assert rel_close(adv_n[s], an) <= 1e-5, e
        assert abs(float(adv_n[s].astype(np.float64).mean())) <= 1e-5
    want = [[raw[offs[e]:offs[e + 1]].astype(np.float64).mean(), raw[offs[e]:offs[e + 1]].astype(np.float64).std(ddof=1)]
            for e in range(len(lens))]
    assert rel_close(mom.cpu().numpy(), want, 1e-9) <= 1e-9


def test_episode_gae_more_than_255_episodes(dev):
    """300 episodes of 2 .. 6 rows: episodes 255 .. 299 run in a second launch, whose seg0 = 255 offsets ep_moments.  Every row of
    ep_moments holds its own episode's (mean, unbiased std) of the raw advantages — float64 arithmetic on at most six float32
    values, hence 1e-9 — so the second launch wrote rows 255 .. 299 and none of the first 255."""
    rng = np.random.default_rng(13)
    lens = [int(n) for n in rng.integers(2, 7, size=300)]
    offs, rew, val, nv, done, dw = _gae_inputs(rng, lens)
    mom = torch.full((len(lens), 2), -7.25, dtype=torch.float64, device=dev)
    adv_n, vt, raw = _run_episode_gae(dev, offs, rew, val, nv, done, dw, mom)
    want = np.empty((len(lens), 2))
    for e in range(len(lens)):
        s = slice(offs[e], offs[e + 1])
        a, v, an = _compute_advantage(rew[s], done[s], dw[s], val[s], nv[s], 0.995, 0.95)
        assert np.array_equal(raw[s], a) and np.array_equal(vt[s], v), e
        assert rel_close(adv_n[s], an) <= 1e-5, e
        want[e] = a.astype(np.float64).mean(), a.astype(np.float64).std(ddof=1)
    got = mom.cpu().numpy()
    assert rel_close(got[255:], want[255:], 1e-9) <= 1e-9
    assert rel_close(got[:255], want[:255], 1e-9) <= 1e-9


def _ref_losses(logits, value, aux, act, old_logp, adv, vt, offs):
    """ppg_rnn_lunarlander.py:330-393 per episode, float32 torch autograd; minibatch loss = mean over episodes."""
    z = torch.from_numpy(logits).requires_grad_(True)
    v = torch.from_numpy(value).requires_grad_(True)
    za = torch.from_numpy(logits.copy()).requires_grad_(True)
    va = torch.from_numpy(aux).requires_grad_(True)
    G = len(offs) - 1
    pol, auxl, m_pol, m_aux = 0, 0, [], []
    for e in range(G):
        s = slice(int(offs[e]), int(offs[e + 1]))
        a = torch.from_numpy(act[s]).long()
        olp, ad, vte = (torch.from_numpy(x[s]).view(-1, 1) for x in (old_logp, adv, vt))
        dist = torch.distributions.Categorical(torch.softmax(z[s], -1))
        ratio = torch.exp(dist.log_prob(a).view(-1, 1) - olp)
        s1, s2 = ratio * ad, torch.clamp(ratio, 1 - CLIP, 1 + CLIP) * ad
        ms = torch.min(s1, s2)
        clip_loss = -torch.mean(torch.where(ad < 0, torch.max(ms, DUAL * ad), ms))
        value_loss = torch.nn.functional.mse_loss(vte, v[s].view(-1, 1))
        ent_loss = -dist.entropy().mean()
        loss = clip_loss + VC * value_loss + EC * ent_loss
        pol = pol + loss / G
        m_pol.append([loss.item(), clip_loss.item(), value_loss.item(), ent_loss.item(), ad.mean().item()])
        av = torch.nn.functional.mse_loss(vte, va[s].view(-1, 1))
        lp = torch.distributions.Categorical(torch.softmax(za[s], -1)).log_prob(a).view(-1, 1)
        cl = torch.nn.functional.mse_loss(lp, olp)
        auxl = auxl + (av + BETA * cl) / G
        m_aux.append([av.item(), cl.item(), av.item() + BETA * cl.item()])
    pol.backward()
    auxl.backward()
    return z.grad.numpy(), v.grad.numpy(), np.array(m_pol), za.grad.numpy(), va.grad.numpy(), np.array(m_aux)


SAT0 = (40.0, 0.0, -1.0, 0.5, 0.25, -0.5, 1.0, -2.0)              # p0 >= 1 - eps, the rest <= eps (1e-17 and below)
SAT1 = (-30.0, 25.0, -2.0, 0.0, -1.0, 0.5, -0.5, 0.25)              # p1 rounds to 1, the rest <= 2.3e-11


def _loss_case(rng, lens, A=4):
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    M = int(offs[-1])
    logits = (rng.normal(size=(M, A)) * 1.5).astype(np.float32)
    logits[0] = SAT0[:A]                                              # saturated: p0 >= 1 - eps, the rest <= eps
    act = rng.integers(0, A, size=M).astype(np.int32)
    if M > 1:
        logits[1] = SAT1[:A]
        act[1] = 0                                                    # the taken action clamped at eps
    p = torch.softmax(torch.from_numpy(logits), -1)
    lp = torch.distributions.Categorical(p).log_prob(torch.from_numpy(act).long()).numpy()
    old = (lp + rng.normal(size=M) * 0.3).astype(np.float32)
    old[2:6] = lp[2:6]                                                # ratio ~1 (both branches' gradients agree)
    adv = rng.normal(size=M).astype(np.float32)
    adv[6:12] = -np.abs(adv[6:12]) - 0.5                              # adv < 0 with ratio far above 1: the dual clip binds
    old[6:12] = lp[6:12] - 2.0
    value, aux, vt = (rng.normal(size=M).astype(np.float32) for _ in range(3))
    return offs, logits, value, aux, act, old, adv, vt


MANY = [int(n) for n in np.random.default_rng(300).integers(1, 6, size=300)]   # 300 episodes of 1 .. 5 rows: two launches
L56_CASES = ([([37], 4), ([1], 4), ([13, 1, 40, 7], 4)]
             + [([37], A) for A in (2, 3, 6, 8)]                                # float2, scalar (odd and even width), A = 8
             + [([255], 4), ([256], 4), ([257], 4), ([600, 1, 300], 4)]         # one short of / exactly / one past a block turn
             + [(MANY, 4)])
L56_IDS = ["lens0", "lens1", "lens2", "A2", "A3", "A6", "A8", "n255", "n256", "n257", "n600-1-300", "G300"]


@pytest.mark.parametrize("lens,A", L56_CASES, ids=L56_IDS)
def test_l5_l6_match_torch_autograd(dev, lens, A):
    from gymrl_amd import ops
    rng = np.random.default_rng(len(lens) * 7 + lens[0])
    offs, logits, value, aux, act, old, adv, vt = _loss_case(rng, lens, A)
    if offs[-1] < 12:
        adv[:] = -np.abs(adv) - 0.5
    r_dz, r_dv, r_mp, r_dza, r_dva, r_ma = _ref_losses(logits, value, aux, act, old, adv, vt, offs)
    msum = torch.zeros(5, dtype=torch.float64, device=dev)
    dz, dv, mp = ops.ppg_policy_loss_fwd_bwd(td(logits, dev), td(value, dev), td(act, dev), td(old, dev), td(adv, dev),
                                             td(vt, dev), offs, CLIP, DUAL, VC, EC, metrics_sum=msum)
    asum = torch.zeros(3, dtype=torch.float64, device=dev)
    dza, dva, ma = ops.ppg_aux_loss_fwd_bwd(td(logits, dev), td(aux, dev), td(act, dev), td(old, dev), td(vt, dev), offs,
                                            BETA, metrics_sum=asum)
    scale = float(np.max(np.diff(offs))) * len(lens)                 # gradients are O(1 / (G * n)): compare them at O(1)
    assert rel_close(dz.cpu().numpy() * scale, r_dz * scale) <= 1e-5
    assert rel_close(dv.cpu().numpy() * scale, r_dv * scale) <= 1e-5
    assert rel_close(dza.cpu().numpy() * scale, r_dza * scale) <= 1e-5
    assert rel_close(dva.cpu().numpy() * scale, r_dva * scale) <= 1e-5
    assert rel_close(mp.cpu().numpy(), r_mp) <= 1e-5 and rel_close(ma.cpu().numpy(), r_ma) <= 1e-5
    assert rel_close(msum.cpu().numpy(), r_mp.mean(0)) <= 1e-5 and rel_close(asum.cpu().numpy(), r_ma.mean(0)) <= 1e-5
    if len(lens) > 255:                                              # the second launch's episodes, each against its own reference
        assert mp.shape == (len(lens), 5) and ma.shape == (len(lens), 3)
        assert rel_close(mp.cpu().numpy()[255:], r_mp[255:]) <= 1e-5 and rel_close(ma.cpu().numpy()[255:], r_ma[255:]) <= 1e-5
        tail = slice(int(offs[255]), int(offs[-1]))
        assert dz.cpu().numpy()[tail].any() and dva.cpu().numpy()[tail].all()
    # the saturated rows: no gradient reaches the clamped logs
    if offs[-1] > 1:
        assert not dza.cpu().numpy()[1].any()


def test_minibatch_loss_is_the_mean_of_single_episode_losses(dev):
    from gymrl_amd import ops
    rng = np.random.default_rng(2)
    D = lambda a: td(a, dev)  # noqa: E731
    for lens in ([5, 31, 1, 12], MANY[:256]):                        # G = 256: the last episode is the first of the second launch
        offs, logits, value, aux, act, old, adv, vt = _loss_case(rng, lens)
        dz, dv, mp = ops.ppg_policy_loss_fwd_bwd(D(logits), D(value), D(act), D(old), D(adv), D(vt), offs, CLIP, DUAL, VC, EC)
        dz, dv, mp = dz.cpu().numpy(), dv.cpu().numpy(), mp.cpu().numpy()
        G = len(lens)
        assert mp.shape == (G, 5)
        for e in range(G):
            s = slice(int(offs[e]), int(offs[e + 1]))
            one = [0, int(offs[e + 1] - offs[e])]
            dz1, dv1, mp1 = ops.ppg_policy_loss_fwd_bwd(D(logits[s]), D(value[s]), D(act[s]), D(old[s]), D(adv[s]), D(vt[s]),
                                                        one, CLIP, DUAL, VC, EC)
            assert np.array_equal(mp[e], mp1.cpu().numpy()[0]), e
            assert rel_close(dz[s] * G * one[1], dz1.cpu().numpy() * one[1]) <= 1e-6, e
            assert rel_close(dv[s] * G * one[1], dv1.cpu().numpy() * one[1]) <= 1e-6, e

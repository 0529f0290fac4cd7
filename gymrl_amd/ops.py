"""Thin torch-tensor front-end over the C-ABI (include/gymrl.h).

PyTorch is plumbing here: it owns device memory and the stream; every op below
passes raw device pointers + the current HIP stream to libgymrl_hip.so.  No op
has a CPU path — tensors must live on an MI355X.
"""
import collections
import ctypes as C

import torch

from ._lib import (ACT_NONE, ACT_RELU, ACT_TANH, MLP_MAX_INPUT, MLP_MAX_STAGES, MLP_MAX_WIDTH, ClassicDuelEvalArgs, ClassicEvalArgs, ClassicPpoEvalArgs, DdqnUpdateArgs, EsNoiseArgs, EsPerturbArgs, EsShapeGradArgs, SnesPerturbArgs, SnesTellArgs, DqnActArgs, NdqnActArgs, NdqnCombineArgs, NdqnUpdateArgs, DqnUpdateArgs, DsacActArgs, DsacUpdateArgs, GaeOnline,
                   LunarCollectArgs, LunarEvalArgs, PendulumPpoEvalArgs, RolloutPendulumArgs, MlpDesc, MlpPackStackArgs, MlprnnParams, AcrobotNetEvalArgs, MountainCarEvalArgs, MountainCarNetEvalArgs, PPOCfg, PPOFullCfg, RainbowActArgs, RainbowUpdateArgs, RolloutLunarArgs, SacActArgs, SacUpdateArgs,
                   TabularTrainArgs, Td3ActArgs, Td3UpdateArgs, check, lib)

_vp = C.c_void_p


def _ptr(t, dtype=None, allow_none=False):
    if t is None:
        if allow_none:
            return _vp(None)
        raise ValueError("tensor required")
    if not t.is_cuda:
        raise RuntimeError("gymrl_amd ops run on the MI355X only: got a CPU tensor (there is no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous")
    return _vp(t.data_ptr())


def _stream():
    return _vp(torch.cuda.current_stream().cuda_stream)


def device_ok():
    return bool(lib().gymrl_device_ok())


# ------------------------------------------------------------------ GAE -----
def gae_workspace(T, N, device):
    nbytes = lib().gymrl_gae_workspace_bytes(T, N)
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def reduce_workspace(device):
    return torch.empty(int(lib().gymrl_reduce_workspace_bytes()), dtype=torch.uint8, device=device)


def gae(rew, val, done, next_val, gamma, lam, adv_out=None, ret_out=None, moments_out=None, variant=1,
        workspace=None):
    """G1 (ppo_lunarlander.py:179-196) over a [T][N] slab.  Returns (adv, ret)."""
    T, N = rew.shape
    adv_out = torch.empty_like(rew) if adv_out is None else adv_out
    ret_out = torch.empty_like(rew) if ret_out is None else ret_out
    if workspace is None and (variant == 1 or moments_out is not None):
        workspace = gae_workspace(T, N, rew.device)
    check(lib().gymrl_gae(_ptr(rew, torch.float32), _ptr(val, torch.float32), _ptr(done, torch.uint8), _ptr(next_val, torch.float32), T, N, gamma,
                          lam, _ptr(adv_out, torch.float32), _ptr(ret_out, torch.float32), _ptr(moments_out, torch.float64, True), variant,
                          _ptr(workspace, None, True), _stream()), "gymrl_gae")
    return adv_out, ret_out


def gae_dw(rew, val, next_val, done, dw, gamma, lam, moments_out=None, workspace=None):
    """G2 (utils/buffer.py:21-35).  Returns (adv, v_target)."""
    T, N = rew.shape
    adv, vt = torch.empty_like(rew), torch.empty_like(rew)
    if workspace is None and moments_out is not None:
        workspace = gae_workspace(T, N, rew.device)
    check(lib().gymrl_gae_dw(_ptr(rew, torch.float32), _ptr(val, torch.float32), _ptr(next_val, torch.float32), _ptr(done, torch.uint8),
                             _ptr(dw, torch.uint8), T, N, gamma, lam, _ptr(adv), _ptr(vt), _ptr(moments_out, torch.float64, True),
                             _ptr(workspace, None, True), _stream()), "gymrl_gae_dw")
    return adv, vt


def gae_decoupled_workspace(T, N, device):
    nbytes = lib().gymrl_gae_decoupled_workspace_bytes(T, N)
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def gae_decoupled(rew, val, done, next_val, gamma, lam_actor, lam_critic, variant=0, workspace=None, adv_out=None,
                  ret_out=None):
    """G3 (ppo_full_lunarlander.py:507-535).  Returns (adv_actor, returns).  variant 1 / 2: time-blocked scan
    (2: chunk maps composed during the rollout), needs gae_decoupled_workspace(T, N)."""
    T, N = rew.shape
    adv = torch.empty_like(rew) if adv_out is None else adv_out
    ret = torch.empty_like(rew) if ret_out is None else ret_out
    if variant and workspace is None:
        workspace = gae_decoupled_workspace(T, N, rew.device)
    check(lib().gymrl_gae_decoupled(_ptr(rew, torch.float32), _ptr(val, torch.float32), _ptr(done, torch.uint8), _ptr(next_val, torch.float32), T, N,
                                    gamma, lam_actor, lam_critic, _ptr(adv), _ptr(ret), variant, _ptr(workspace, None, True), _stream()),
          "gymrl_gae_decoupled")
    return adv, ret


def moments(x, out=None, workspace=None):
    out = torch.empty(3, dtype=torch.float64, device=x.device) if out is None else out
    workspace = reduce_workspace(x.device) if workspace is None else workspace
    check(lib().gymrl_moments(_ptr(x, torch.float32), x.numel(), _ptr(out, torch.float64), _ptr(workspace), _stream()), "gymrl_moments")
    return out


def normalize_(x, mom, ddof=0, eps=1e-8):
    check(lib().gymrl_normalize(_ptr(x, torch.float32), x.numel(), _ptr(mom, torch.float64), ddof, eps, _stream()), "gymrl_normalize")
    return x


# ------------------------------------------------------------ categorical ---
def gae_online(rew_prev, done_prev, val_prev, running, workspace, t_prev, T, gamma, lam, lam2=0.0, running2=None):
    """Descriptor for the producer-side GAE fusion (gymrl_gae_online): rows t-1 of the slab.  lam2 / running2: the
    decoupled-lambda mode of G3 (lam = lam_actor, lam2 = lam_critic)."""
    return GaeOnline(rew_prev.data_ptr(), done_prev.data_ptr(), val_prev.data_ptr(), running.data_ptr(),
                     workspace.data_ptr(), int(t_prev), int(T), float(gamma), float(lam), float(lam2),
                     running2.data_ptr() if running2 is not None else None)


def gae_online_flush(online, val_cur):
    check(lib().gymrl_gae_online_flush(C.byref(online), _ptr(val_cur, torch.float32), val_cur.numel(), _stream()), "gymrl_gae_online_flush")


def categorical_sample(logits, value=None, noise_exp=None, seed=0, counter=0, env_id0=0, deterministic=False,
                       act_out=None, logp_out=None, ent_out=None, value_out=None, online=None):
    """P2 (ppo_lunarlander.py:92-104).  Returns (action i32[N], logp, entropy, value_out)."""
    n, A = logits.shape
    dev = logits.device
    act_out = torch.empty(n, dtype=torch.int32, device=dev) if act_out is None else act_out
    logp_out = torch.empty(n, dtype=torch.float32, device=dev) if logp_out is None else logp_out
    ent_out = torch.empty(n, dtype=torch.float32, device=dev) if ent_out is None else ent_out
    if value is not None and value_out is None:
        value_out = torch.empty(n, dtype=torch.float32, device=dev)
    check(lib().gymrl_categorical_sample(_ptr(logits, torch.float32), _ptr(value, torch.float32, True), _ptr(noise_exp, torch.float32, True), seed,
                                         counter, env_id0, n, A, int(deterministic), _ptr(act_out, torch.int32), _ptr(logp_out),
                                         _ptr(ent_out, None, True), _ptr(value_out, None, True), C.byref(online) if online is not None else None,
                                         _stream()), "gymrl_categorical_sample")
    return act_out, logp_out, ent_out, value_out


GAUSS_MAX_ACT = 8              # gymrl_gaussian_sample / gymrl_ppo_gauss_loss_fwd_bwd: 1 <= A <= 8


def _need_dev(who, **tensors):
    """The Gaussian entry points' wrappers: a CPU tensor is refused before any pointer is read."""
    for name, t in tensors.items():
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"{who}: {name} is a CPU tensor; gymrl_amd ops run on the MI355X only (no CPU fallback)")


def gaussian_sample_shape_ok(N, A):
    """What gymrl_gaussian_sample takes: N >= 0 rows of 1..8 action components."""
    return N >= 0 and 1 <= A <= GAUSS_MAX_ACT


def gaussian_sample(mu, log_std, value=None, noise_normal=None, seed=0, counter=0, env_id0=0, deterministic=False, act_out=None,
                    logp_out=None, ent_out=None, value_out=None, online=None):
    """The Gaussian policy's draw (include/gymrl.h "Gaussian policy"): mu f32[N, A], log_std f32[A] -> (action f32[N, A], logp,
    entropy, value_out).  noise_normal f32[N, A]: explicit N(0, 1) draws (parity mode)."""
    if mu.dim() != 2 or not gaussian_sample_shape_ok(*mu.shape):
        raise ValueError(f"gaussian_sample: mu is f32[N, A] with 1 <= A <= {GAUSS_MAX_ACT}, not {tuple(mu.shape)}")
    n, A = mu.shape
    if tuple(log_std.shape) != (A,):
        raise ValueError(f"gaussian_sample: log_std is f32[A] = {(A,)}, not {tuple(log_std.shape)}")
    for name, t, shape in (("value", value, (n,)), ("noise_normal", noise_normal, (n, A)), ("act_out", act_out, (n, A)),
                           ("logp_out", logp_out, (n,)), ("ent_out", ent_out, (n,)), ("value_out", value_out, (n,))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"gaussian_sample: {name} is {shape}, not {tuple(t.shape)}")
    if online is not None and value is None:
        raise ValueError("gaussian_sample: the online GAE composition needs the values")
    _need_dev("gaussian_sample", mu=mu, log_std=log_std, value=value, noise_normal=noise_normal, act_out=act_out, logp_out=logp_out,
              ent_out=ent_out, value_out=value_out)
    dev = mu.device
    act_out = torch.empty(n, A, dtype=torch.float32, device=dev) if act_out is None else act_out
    logp_out = torch.empty(n, dtype=torch.float32, device=dev) if logp_out is None else logp_out
    ent_out = torch.empty(n, dtype=torch.float32, device=dev) if ent_out is None else ent_out
    if value is not None and value_out is None:
        value_out = torch.empty(n, dtype=torch.float32, device=dev)
    check(lib().gymrl_gaussian_sample(_ptr(mu, torch.float32), _ptr(log_std, torch.float32), _ptr(value, torch.float32, True),
                                      _ptr(noise_normal, torch.float32, True), seed, counter, env_id0, n, A, int(deterministic),
                                      _ptr(act_out, torch.float32), _ptr(logp_out, torch.float32), _ptr(ent_out, torch.float32, True),
                                      _ptr(value_out, torch.float32, True), C.byref(online) if online is not None else None, _stream()),
          "gymrl_gaussian_sample")
    return act_out, logp_out, ent_out, value_out


# --------------------------------------------------------------- PPO loss ---
_ws_cache = {}


def _reduce_ws(device):
    key = (device.type, device.index)
    if key not in _ws_cache:
        _ws_cache[key] = reduce_workspace(device)
    return _ws_cache[key]


def ppo_loss_fwd_bwd(logits, value, act, logp_old, adv, ret, cfg, idx=None, adv_moments=None, dlogits_out=None,
                     dvalue_out=None, metrics_sum=None, workspace=None):
    """L1+L2 (ppo_lunarlander.py:278-322).  cfg = (clip_eps, dual_clip, value_coef, entropy_coef)."""
    B, A = logits.shape
    dlogits_out = torch.empty_like(logits) if dlogits_out is None else dlogits_out
    dvalue_out = torch.empty(B, dtype=torch.float32, device=logits.device) if dvalue_out is None else dvalue_out
    c = PPOCfg(*cfg)
    if metrics_sum is not None and workspace is None:
        workspace = _reduce_ws(logits.device)
    check(lib().gymrl_ppo_loss_fwd_bwd(_ptr(logits, torch.float32), _ptr(value, torch.float32), _ptr(idx, torch.int32, True), _ptr(act, torch.int32),
                                       _ptr(logp_old, torch.float32), _ptr(adv, torch.float32), _ptr(ret, torch.float32),
                                       _ptr(adv_moments, torch.float64, True), B, A, C.byref(c), _ptr(dlogits_out), _ptr(dvalue_out),
                                       _ptr(metrics_sum, torch.float64, True), _ptr(workspace, None, True), _stream()), "gymrl_ppo_loss_fwd_bwd")
    return dlogits_out, dvalue_out


def ppo_gauss_loss_shape_ok(B, A):
    """What gymrl_ppo_gauss_loss_fwd_bwd takes: B >= 0 rows of 1..8 action components."""
    return B >= 0 and 1 <= A <= GAUSS_MAX_ACT


def ppo_gauss_loss_workspace(B, A, device):
    """The float64 segment table of the log_std gradient, f64[ceil(B / 256), A] (gymrl_ppo_gauss_loss_workspace_bytes)."""
    return torch.empty(max(int(lib().gymrl_ppo_gauss_loss_workspace_bytes(B, A)) // 8, 1), dtype=torch.float64, device=device)


def ppo_gauss_loss_fwd_bwd(mu, log_std, value, act, logp_old, adv, ret, cfg, idx=None, adv_moments=None, dmu_out=None, dvalue_out=None,
                           dlog_std_out=None, metrics_sum=None, workspace=None, dls_workspace=None, grid_blocks=0):
    """L1 under the Gaussian policy (include/gymrl.h): mu f32[B, A], log_std f32[A], value f32[B]; act f32[M, A], logp_old / adv /
    ret f32[M] read at idx[b] (or at b: M >= B) -> (dmu f32[B, A], dvalue f32[B], dlog_std f32[A]).  cfg = (clip_eps, dual_clip,
    value_coef, entropy_coef).  grid_blocks: 0 = the default grid; dlog_std carries the same bits under every grid."""
    if mu.dim() != 2 or not ppo_gauss_loss_shape_ok(*mu.shape):
        raise ValueError(f"ppo_gauss_loss_fwd_bwd: mu is f32[B, A] with 1 <= A <= {GAUSS_MAX_ACT}, not {tuple(mu.shape)}")
    B, A = mu.shape
    if tuple(log_std.shape) != (A,) or tuple(value.shape) != (B,):
        raise ValueError(f"ppo_gauss_loss_fwd_bwd: log_std is f32[{A}] and value f32[{B}], not {tuple(log_std.shape)} and {tuple(value.shape)}")
    if act.dim() != 2 or act.shape[1] != A:
        raise ValueError(f"ppo_gauss_loss_fwd_bwd: act is f32[M, {A}], not {tuple(act.shape)}")
    M = act.shape[0]
    for name, t in (("logp_old", logp_old), ("adv", adv), ("ret", ret)):
        if tuple(t.shape) != (M,):
            raise ValueError(f"ppo_gauss_loss_fwd_bwd: {name} is f32[M] = {(M,)}, not {tuple(t.shape)}")
    if (idx is None and M < B) or (idx is not None and tuple(idx.shape) != (B,)):
        raise ValueError("ppo_gauss_loss_fwd_bwd: idx is i32[B], and without it the stored rows are at least B")
    for name, t, shape in (("adv_moments", adv_moments, (3,)), ("dmu_out", dmu_out, (B, A)), ("dvalue_out", dvalue_out, (B,)),
                           ("dlog_std_out", dlog_std_out, (A,)), ("metrics_sum", metrics_sum, (5,))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"ppo_gauss_loss_fwd_bwd: {name} is {shape}, not {tuple(t.shape)}")
    if grid_blocks < 0 or (grid_blocks and workspace is not None and metrics_sum is None):
        raise ValueError("ppo_gauss_loss_fwd_bwd: grid_blocks is >= 0, and 0 where `workspace` is the caller's table of metric partials")
    if dls_workspace is not None and dls_workspace.numel() * dls_workspace.element_size() < int(lib().gymrl_ppo_gauss_loss_workspace_bytes(B, A)):
        raise ValueError("ppo_gauss_loss_fwd_bwd: dls_workspace is smaller than gymrl_ppo_gauss_loss_workspace_bytes(B, A)")
    _need_dev("ppo_gauss_loss_fwd_bwd", mu=mu, log_std=log_std, value=value, act=act, logp_old=logp_old, adv=adv, ret=ret, idx=idx,
              adv_moments=adv_moments, dmu_out=dmu_out, dvalue_out=dvalue_out, dlog_std_out=dlog_std_out, metrics_sum=metrics_sum,
              workspace=workspace, dls_workspace=dls_workspace)
    dev = mu.device
    dmu_out = torch.empty_like(mu) if dmu_out is None else dmu_out
    dvalue_out = torch.empty(B, dtype=torch.float32, device=dev) if dvalue_out is None else dvalue_out
    dlog_std_out = torch.empty(A, dtype=torch.float32, device=dev) if dlog_std_out is None else dlog_std_out
    if metrics_sum is not None and workspace is None:
        workspace = _reduce_ws(dev)
    if dls_workspace is None:
        dls_workspace = ppo_gauss_loss_workspace(B, A, dev)
    c = PPOCfg(*cfg)
    check(lib().gymrl_ppo_gauss_loss_fwd_bwd(_ptr(mu, torch.float32), _ptr(log_std, torch.float32), _ptr(value, torch.float32),
                                             _ptr(idx, torch.int32, True), _ptr(act, torch.float32), _ptr(logp_old, torch.float32),
                                             _ptr(adv, torch.float32), _ptr(ret, torch.float32), _ptr(adv_moments, torch.float64, True), B, A,
                                             C.byref(c), _ptr(dmu_out, torch.float32), _ptr(dvalue_out, torch.float32),
                                             _ptr(dlog_std_out, torch.float32), _ptr(metrics_sum, torch.float64, True),
                                             _ptr(workspace, None, True), _ptr(dls_workspace), int(grid_blocks), _stream()),
          "gymrl_ppo_gauss_loss_fwd_bwd")
    return dmu_out, dvalue_out, dlog_std_out


def ppo_full_loss_fwd_bwd(logits, value, act, logp_old, ent_old, adv, ret, cfg, idx=None, dlogits_out=None,
                          dvalue_out=None, metrics_sum=None, workspace=None, corr_mul=None, entropy_coef_dev=None):
    """L3 (ppo_full_lunarlander.py:575-652).  entropy_coef_dev: f32[1] on the device that overrides cfg's entropy coefficient
    (a captured graph replayed across updates)."""
    B, A = logits.shape
    dlogits_out = torch.empty_like(logits) if dlogits_out is None else dlogits_out
    dvalue_out = torch.empty(B, dtype=torch.float32, device=logits.device) if dvalue_out is None else dvalue_out
    c = PPOFullCfg(*cfg)
    c.entropy_coef_dev = None if entropy_coef_dev is None else _ptr(entropy_coef_dev, torch.float32).value
    if metrics_sum is not None and workspace is None:
        workspace = _reduce_ws(logits.device)
    check(lib().gymrl_ppo_full_loss_fwd_bwd(_ptr(logits, torch.float32), _ptr(value, torch.float32), _ptr(idx, torch.int32, True),
                                            _ptr(act, torch.int32), _ptr(logp_old, torch.float32), _ptr(ent_old, torch.float32),
                                            _ptr(adv, torch.float32), _ptr(ret, torch.float32), B, A, C.byref(c), _ptr(corr_mul, torch.float32, True),
                                            _ptr(dlogits_out), _ptr(dvalue_out), _ptr(metrics_sum, torch.float64, True), _ptr(workspace, None, True),
                                            _stream()), "gymrl_ppo_full_loss_fwd_bwd")
    return dlogits_out, dvalue_out


def ppo_rnn_loss_fwd_bwd(logits, value, act, logp_old, ent_old, val_old, adv, ret, cfg, idx=None, metrics_sum=None,
                         corr_mul=None):
    """L4 (ppo_lstm_lunarlander.py:716-776): masked means + clipped value loss.  metrics_sum f64[10]."""
    B, A = logits.shape
    dlogits, dvalue = torch.empty_like(logits), torch.empty(B, dtype=torch.float32, device=logits.device)
    c = PPOFullCfg(*cfg)
    check(lib().gymrl_ppo_rnn_loss_fwd_bwd(_ptr(logits, torch.float32), _ptr(value, torch.float32), _ptr(idx, torch.int32, True),
                                           _ptr(act, torch.int32), _ptr(logp_old, torch.float32), _ptr(ent_old, torch.float32),
                                           _ptr(val_old, torch.float32), _ptr(adv, torch.float32), _ptr(ret, torch.float32), B, A, C.byref(c),
                                           _ptr(corr_mul, torch.float32, True), _ptr(dlogits), _ptr(dvalue), _ptr(metrics_sum, torch.float64, True),
                                           _ptr(_reduce_ws(logits.device)), _stream()), "gymrl_ppo_rnn_loss_fwd_bwd")
    return dlogits, dvalue


def gru_cell_fwd(gi, gh, h, out=None):
    B, H = h.shape
    out = torch.empty_like(h) if out is None else out
    check(lib().gymrl_gru_cell_fwd(_ptr(gi, torch.float32), _ptr(gh, torch.float32), _ptr(h, torch.float32), B, H, _ptr(out, torch.float32), _stream()),
          "gymrl_gru_cell_fwd")
    return out


def gru_cell_bwd(gi, gh, h, dh_out):
    B, H = h.shape
    dgi, dgh, dh = torch.empty_like(gi), torch.empty_like(gh), torch.empty_like(h)
    check(lib().gymrl_gru_cell_bwd(_ptr(gi, torch.float32), _ptr(gh, torch.float32), _ptr(h, torch.float32), _ptr(dh_out, torch.float32), B, H,
                                   _ptr(dgi), _ptr(dgh), _ptr(dh), _stream()), "gymrl_gru_cell_bwd")
    return dgi, dgh, dh


def _host_i32(x):
    vals = [int(v) for v in (x.tolist() if hasattr(x, "tolist") else x)]
    return (C.c_int32 * max(len(vals), 1))(*vals), len(vals)


def _host_i64(x):
    vals = [int(v) for v in (x.tolist() if hasattr(x, "tolist") else x)]
    return (C.c_int64 * max(len(vals), 1))(*vals), len(vals)


def _need_shape(t, shape, name):
    """The host-side lengths / offsets steer the kernels' addressing: every tensor they index must have the shape
    they imply (a mismatch would read or write past its end)."""
    if t is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")


def _gru_seq_shapes(gi, W_hh, b_hh, h0, lens_len, T, B, H, **more):
    if gi.dim() != 3 or gi.shape[2] % 3:
        raise ValueError(f"gi: expected [T, B, 3H], got {tuple(gi.shape)}")
    if lens_len != B:
        raise ValueError(f"lengths has {lens_len} entries for {B} episodes")
    _need_shape(W_hh, (3 * H, H), "W_hh")
    _need_shape(b_hh, (3 * H,), "b_hh")
    _need_shape(h0, (B, H), "h0")
    for name, (t, shape) in more.items():
        _need_shape(t, shape, name)


def _segments(offsets, M, what):
    offs, n1 = _host_i64(offsets)
    if n1 < 1 or offs[n1 - 1] != M:
        raise ValueError(f"{what}: offsets must end at the {M} stored rows (got {list(offs)[-1:] if n1 else []})")
    return offs, n1 - 1


def gru_seq_fwd(gi, W_hh, b_hh, lengths, h0=None, h_seq=None, h_last=None):
    """The GRU over whole episodes in one launch (gymrl_gru_seq_fwd).  gi f32[T,B,3H] time-major, lengths: host ints [B].
    Returns (h_seq f32[T,B,H], zero past each length; h_last f32[B,H])."""
    T, B, H3 = gi.shape
    H = H3 // 3
    lens, nb = _host_i32(lengths)
    _gru_seq_shapes(gi, W_hh, b_hh, h0, nb, T, B, H, h_seq=(h_seq, (T, B, H)), h_last=(h_last, (B, H)))
    h_seq = torch.empty(T, B, H, dtype=torch.float32, device=gi.device) if h_seq is None else h_seq
    h_last = torch.empty(B, H, dtype=torch.float32, device=gi.device) if h_last is None else h_last
    check(lib().gymrl_gru_seq_fwd(_ptr(gi, torch.float32), _ptr(W_hh, torch.float32), _ptr(b_hh, torch.float32),
                                  _ptr(h0, torch.float32, True), lens, T, B, H, _ptr(h_seq, torch.float32),
                                  _ptr(h_last, torch.float32), _stream()), "gymrl_gru_seq_fwd")
    return h_seq, h_last


def gru_seq_bwd(gi, W_hh, b_hh, h_seq, lengths, d_hseq=None, d_hlast=None, h0=None, need_dh0=True, dgi=None, dgh=None,
                dh0=None):
    """Reverse recurrence of gru_seq_fwd (gymrl_gru_seq_bwd).  Returns (dgi, dgh f32[T,B,3H], dh0 f32[B,H] or None);
    dgi, dgh, dh0: the caller's buffers to write them into."""
    T, B, H3 = gi.shape
    H = H3 // 3
    lens, nb = _host_i32(lengths)
    if dh0 is not None and not need_dh0:
        raise ValueError("dh0 given with need_dh0=False")
    _gru_seq_shapes(gi, W_hh, b_hh, h0, nb, T, B, H, h_seq=(h_seq, (T, B, H)), d_hseq=(d_hseq, (T, B, H)),
                    d_hlast=(d_hlast, (B, H)), dgi=(dgi, (T, B, H3)), dgh=(dgh, (T, B, H3)), dh0=(dh0, (B, H)))
    dgi = torch.empty_like(gi) if dgi is None else dgi
    dgh = torch.empty_like(gi) if dgh is None else dgh
    if need_dh0 and dh0 is None:
        dh0 = torch.empty(B, H, dtype=torch.float32, device=gi.device)
    check(lib().gymrl_gru_seq_bwd(_ptr(gi, torch.float32), _ptr(W_hh, torch.float32), _ptr(b_hh, torch.float32),
                                  _ptr(h0, torch.float32, True), _ptr(h_seq, torch.float32),
                                  _ptr(d_hseq, torch.float32, True), _ptr(d_hlast, torch.float32, True), lens, T, B, H,
                                  _ptr(dgi, torch.float32), _ptr(dgh, torch.float32), _ptr(dh0, torch.float32, True), _stream()),
          "gymrl_gru_seq_bwd")
    return dgi, dgh, dh0


def lstm_cell_fwd(gi, gh, c):
    """The pointwise half of nn.LSTM's cell (gymrl_lstm_cell_fwd).  gi, gh f32[B,4H], c f32[B,H] -> (h', c')."""
    B, H = c.shape
    _need_shape(gi, (B, 4 * H), "gi")
    _need_shape(gh, (B, 4 * H), "gh")
    h_out, c_out = torch.empty_like(c), torch.empty_like(c)
    check(lib().gymrl_lstm_cell_fwd(_ptr(gi, torch.float32), _ptr(gh, torch.float32), _ptr(c, torch.float32), B, H,
                                    _ptr(h_out, torch.float32), _ptr(c_out, torch.float32), _stream()), "gymrl_lstm_cell_fwd")
    return h_out, c_out


def lstm_cell_bwd(gi, gh, c, dh_out, dc_out=None):
    """Backward of lstm_cell_fwd (gymrl_lstm_cell_bwd).  Returns (dgates f32[B,4H] = dgi = dgh, dc f32[B,H])."""
    B, H = c.shape
    _need_shape(gi, (B, 4 * H), "gi")
    _need_shape(gh, (B, 4 * H), "gh")
    _need_shape(dh_out, (B, H), "dh_out")
    _need_shape(dc_out, (B, H), "dc_out")
    dgates, dc = torch.empty_like(gi), torch.empty_like(c)
    check(lib().gymrl_lstm_cell_bwd(_ptr(gi, torch.float32), _ptr(gh, torch.float32), _ptr(c, torch.float32),
                                    _ptr(dh_out, torch.float32), _ptr(dc_out, torch.float32, True), B, H, _ptr(dgates), _ptr(dc),
                                    _stream()), "gymrl_lstm_cell_bwd")
    return dgates, dc


def _lstm_seq_shapes(gi, W_hh, b_hh, h0, c0, lens_len, T, B, H, **more):
    if gi.dim() != 3 or gi.shape[2] % 4:
        raise ValueError(f"gi: expected [T, B, 4H], got {tuple(gi.shape)}")
    if lens_len != B:
        raise ValueError(f"lengths has {lens_len} entries for {B} rows")
    _need_shape(W_hh, (4 * H, H), "W_hh")
    _need_shape(b_hh, (4 * H,), "b_hh")
    _need_shape(h0, (B, H), "h0")
    _need_shape(c0, (B, H), "c0")
    for name, (t, shape) in more.items():
        _need_shape(t, shape, name)


def lstm_seq_fwd(gi, W_hh, b_hh, lengths, h0=None, c0=None, h_seq=None, c_seq=None, h_last=None, c_last=None):
    """The LSTM recurrence in one launch (gymrl_lstm_seq_fwd).  gi f32[T,B,4H] time-major, lengths: host ints [B].
    Returns (h_seq, c_seq f32[T,B,H], zero past each length; h_last, c_last f32[B,H]); each may be given as the caller's
    buffer to write into."""
    if gi.dim() != 3:
        raise ValueError(f"gi: expected [T, B, 4H], got {tuple(gi.shape)}")
    T, B, H4 = gi.shape
    H = H4 // 4
    lens, nb = _host_i32(lengths)
    _lstm_seq_shapes(gi, W_hh, b_hh, h0, c0, nb, T, B, H, h_seq=(h_seq, (T, B, H)), c_seq=(c_seq, (T, B, H)),
                     h_last=(h_last, (B, H)), c_last=(c_last, (B, H)))
    h_seq, c_seq = (torch.empty(T, B, H, dtype=torch.float32, device=gi.device) if t is None else t for t in (h_seq, c_seq))
    h_last, c_last = (torch.empty(B, H, dtype=torch.float32, device=gi.device) if t is None else t for t in (h_last, c_last))
    check(lib().gymrl_lstm_seq_fwd(_ptr(gi, torch.float32), _ptr(W_hh, torch.float32), _ptr(b_hh, torch.float32),
                                   _ptr(h0, torch.float32, True), _ptr(c0, torch.float32, True), lens, T, B, H,
                                   _ptr(h_seq, torch.float32), _ptr(c_seq, torch.float32), _ptr(h_last, torch.float32),
                                   _ptr(c_last, torch.float32), _stream()), "gymrl_lstm_seq_fwd")
    return h_seq, c_seq, h_last, c_last


def lstm_seq_bwd(gi, W_hh, b_hh, h_seq, c_seq, lengths, d_hseq=None, d_hlast=None, d_clast=None, h0=None, c0=None,
                 need_d0=True, dgates=None, dh0=None, dc0=None):
    """Reverse recurrence of lstm_seq_fwd (gymrl_lstm_seq_bwd).  Returns (dgates f32[T,B,4H] = dgi = dgh, dh0, dc0
    f32[B,H] or None); dgates, dh0, dc0: the caller's buffers to write them into."""
    if gi.dim() != 3:
        raise ValueError(f"gi: expected [T, B, 4H], got {tuple(gi.shape)}")
    T, B, H4 = gi.shape
    H = H4 // 4
    lens, nb = _host_i32(lengths)
    if not need_d0 and (dh0 is not None or dc0 is not None):
        raise ValueError("dh0 / dc0 given with need_d0=False")
    _lstm_seq_shapes(gi, W_hh, b_hh, h0, c0, nb, T, B, H, h_seq=(h_seq, (T, B, H)), c_seq=(c_seq, (T, B, H)),
                     d_hseq=(d_hseq, (T, B, H)), d_hlast=(d_hlast, (B, H)), d_clast=(d_clast, (B, H)),
                     dgates=(dgates, (T, B, H4)), dh0=(dh0, (B, H)), dc0=(dc0, (B, H)))
    dgates = torch.empty_like(gi) if dgates is None else dgates
    if need_d0:
        dh0, dc0 = (torch.empty(B, H, dtype=torch.float32, device=gi.device) if t is None else t for t in (dh0, dc0))
    check(lib().gymrl_lstm_seq_bwd(_ptr(gi, torch.float32), _ptr(W_hh, torch.float32), _ptr(b_hh, torch.float32),
                                   _ptr(h0, torch.float32, True), _ptr(c0, torch.float32, True), _ptr(h_seq, torch.float32),
                                   _ptr(c_seq, torch.float32), _ptr(d_hseq, torch.float32, True),
                                   _ptr(d_hlast, torch.float32, True), _ptr(d_clast, torch.float32, True), lens, T, B, H,
                                   _ptr(dgates, torch.float32), _ptr(dh0, torch.float32, True), _ptr(dc0, torch.float32, True),
                                   _stream()), "gymrl_lstm_seq_bwd")
    return dgates, dh0, dc0


def episode_gae(rew, val, next_val, done, dw, offsets, gamma, lam, want_raw=False, ep_moments=None):
    """EpisodeBuffer.compute_advantage per episode (ppg_rnn_lunarlander.py:198-215) over episodes stored back to back;
    offsets: host ints [E+1].  Returns (adv_norm, v_target, adv_raw or None)."""
    M = rew.numel()
    offs, E = _segments(offsets, M, "episode_gae")
    for name, t in (("val", val), ("next_val", next_val), ("done", done), ("dw", dw)):
        _need_shape(t, (M,), name)
    _need_shape(ep_moments, (E, 2), "ep_moments")
    n1 = E + 1
    adv_norm, vt = torch.empty_like(rew), torch.empty_like(rew)
    raw = torch.empty_like(rew) if want_raw else None
    check(lib().gymrl_episode_gae(_ptr(rew, torch.float32), _ptr(val, torch.float32), _ptr(next_val, torch.float32),
                                  _ptr(done, torch.uint8), _ptr(dw, torch.uint8), offs, n1 - 1, float(gamma), float(lam),
                                  _ptr(raw, torch.float32, True), _ptr(adv_norm), _ptr(vt),
                                  _ptr(ep_moments, torch.float64, True), _stream()), "gymrl_episode_gae")
    return adv_norm, vt, raw


def ppg_policy_loss_fwd_bwd(logits, value, act, old_logp, adv, v_target, offsets, clip, dual_clip, val_coef, ent_coef,
                            metrics_sum=None):
    """L5 (ppg_rnn_lunarlander.py:330-370) over G episodes.  Returns (dlogits, dvalue, metrics_ep f64[G,5] =
    (loss, clip_loss, value_loss, entropy_loss, adv mean) per episode)."""
    M, A = logits.shape
    offs, G = _segments(offsets, M, "ppg_policy_loss_fwd_bwd")
    for name, t in (("value", value), ("act", act), ("old_logp", old_logp), ("adv", adv), ("v_target", v_target)):
        _need_shape(t, (M,), name)
    _need_shape(metrics_sum, (5,), "metrics_sum")
    dlogits, dvalue = torch.empty_like(logits), torch.empty(M, dtype=torch.float32, device=logits.device)
    metrics_ep = torch.empty(max(G, 1), 5, dtype=torch.float64, device=logits.device)
    check(lib().gymrl_ppg_policy_loss_fwd_bwd(_ptr(logits, torch.float32), _ptr(value, torch.float32),
                                              _ptr(act, torch.int32), _ptr(old_logp, torch.float32),
                                              _ptr(adv, torch.float32), _ptr(v_target, torch.float32), offs, G, A,
                                              clip, dual_clip, val_coef, ent_coef, _ptr(dlogits), _ptr(dvalue),
                                              _ptr(metrics_ep), _ptr(metrics_sum, torch.float64, True), _stream()),
          "gymrl_ppg_policy_loss_fwd_bwd")
    return dlogits, dvalue, metrics_ep


def ppg_aux_loss_fwd_bwd(logits, aux_value, act, old_logp, v_target, offsets, beta, metrics_sum=None):
    """L6 (ppg_rnn_lunarlander.py:372-393) over G episodes.  Returns (dlogits, d_aux, metrics_ep f64[G,3] =
    (aux_value_loss, clone_loss, joint) per episode)."""
    M, A = logits.shape
    offs, G = _segments(offsets, M, "ppg_aux_loss_fwd_bwd")
    for name, t in (("aux_value", aux_value), ("act", act), ("old_logp", old_logp), ("v_target", v_target)):
        _need_shape(t, (M,), name)
    _need_shape(metrics_sum, (3,), "metrics_sum")
    dlogits, d_aux = torch.empty_like(logits), torch.empty(M, dtype=torch.float32, device=logits.device)
    metrics_ep = torch.empty(max(G, 1), 3, dtype=torch.float64, device=logits.device)
    check(lib().gymrl_ppg_aux_loss_fwd_bwd(_ptr(logits, torch.float32), _ptr(aux_value, torch.float32),
                                           _ptr(act, torch.int32), _ptr(old_logp, torch.float32),
                                           _ptr(v_target, torch.float32), offs, G, A, beta, _ptr(dlogits), _ptr(d_aux),
                                           _ptr(metrics_ep), _ptr(metrics_sum, torch.float64, True), _stream()),
          "gymrl_ppg_aux_loss_fwd_bwd")
    return dlogits, d_aux, metrics_ep


def mlprnn_params(net):
    """gymrl_mlprnn_params of a PSCN -> MLPRNN -> actor_fc / critic_fc network (ppg_rnn_lunarlander.py:143-176): the
    parameters' own device addresses.  They are views of the flat buffer the optimiser updates in place, so one descriptor
    serves the whole run.  The float4-read weights must be 16-byte aligned (flatten_module aligns every view)."""
    P = MlprnnParams()
    for i, layer in enumerate(net.fc_head.layers):
        lin, act = layer.mlp[0], layer.mlp[1]
        P.pscn_w[i], P.pscn_b[i], P.pscn_a[i] = _addr(lin.weight), _addr(lin.bias), _addr(act.weight)
    P.lin_w, P.lin_b = _addr(net.rnn.rnn_linear.mlp[0].weight), _addr(net.rnn.rnn_linear.mlp[0].bias)
    g = net.rnn.rnn
    P.w_ih, P.b_ih, P.w_hh, P.b_hh = (_addr(t) for t in (g.weight_ih_l0, g.bias_ih_l0, g.weight_hh_l0, g.bias_hh_l0))
    a, c = net.actor_fc.mlp, net.critic_fc.mlp
    P.actor_w1, P.actor_b1, P.actor_a, P.actor_w2, P.actor_b2 = (_addr(t) for t in (a[0].weight, a[0].bias, a[1].weight,
                                                                                  a[2].weight, a[2].bias))
    P.critic_w1, P.critic_b1, P.critic_a, P.critic_w2, P.critic_b2 = (_addr(t) for t in (c[0].weight, c[0].bias, c[1].weight,
                                                                                       c[2].weight, c[2].bias))
    for t in [p for p in net.parameters()]:
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("mlprnn_params: every parameter must be a contiguous f32 device tensor")
    P._device = net.fc_head.layers[0].mlp[0].weight.device       # (where lunar_mlprnn_eval allocates its outputs)
    return P


def mlprnn_act(x, h_in, params, A, live=None, noise_exp=None, seed=0, counter=0, env_id0=0, deterministic=False,
               h_out=None, act_out=None, logp_out=None, value_out=None, probs_out=None):
    """gymrl_mlprnn_act: the network's single-step forward for N envs + the Categorical draw, one launch
    (ppg_rnn_lunarlander.py:311-328).  x f32[N,D], h_in f32[N,64]; h_out may be h_in.  Returns (act i32[N], logp f32[N],
    value f32[N], h_out f32[N,64], probs f32[N,A] or None).  Rows with live == 0 are not written."""
    N, D = x.shape
    dev = x.device
    _need_shape(h_in, (N, 64), "h_in")
    for name, t, shape in (("live", live, (N,)), ("noise_exp", noise_exp, (N, A)), ("h_out", h_out, (N, 64)),
                           ("act_out", act_out, (N,)), ("logp_out", logp_out, (N,)), ("value_out", value_out, (N,)),
                           ("probs_out", probs_out, (N, A))):
        _need_shape(t, shape, name)
    h_out = torch.empty_like(h_in) if h_out is None else h_out
    act_out = torch.empty(N, dtype=torch.int32, device=dev) if act_out is None else act_out
    logp_out = torch.empty(N, dtype=torch.float32, device=dev) if logp_out is None else logp_out
    value_out = torch.empty(N, dtype=torch.float32, device=dev) if value_out is None else value_out
    check(lib().gymrl_mlprnn_act(_ptr(x, torch.float32), _ptr(h_in, torch.float32), C.byref(params), N, D, int(A),
                                 _ptr(live, torch.uint8, True), _ptr(noise_exp, torch.float32, True), seed, counter, env_id0,
                                 int(bool(deterministic)), _ptr(h_out, torch.float32), _ptr(act_out, torch.int32),
                                 _ptr(logp_out, torch.float32), _ptr(value_out, torch.float32),
                                 _ptr(probs_out, torch.float32, True), _stream()), "gymrl_mlprnn_act")
    return act_out, logp_out, value_out, h_out, probs_out


def rnd_reward(predict, target, rew_inout=None, rnd_out=None):
    B, E = predict.shape
    check(lib().gymrl_rnd_reward(_ptr(predict, torch.float32), _ptr(target, torch.float32), B, E, _ptr(rew_inout, torch.float32, True),
                                 _ptr(rnd_out, torch.float32, True), _stream()), "gymrl_rnd_reward")


def loss_blocks(B):
    return int(lib().gymrl_loss_blocks(B))


def reduce_rows(partials, rows, blocks_per_row, K):
    """[rows, blocks_per_row, K] f64 block partials -> [rows, K] sums (one launch)."""
    out = torch.empty(rows, K, dtype=torch.float64, device=partials.device)
    check(lib().gymrl_reduce_rows(_ptr(partials, torch.float64), rows, blocks_per_row, K, _ptr(out), _stream()), "gymrl_reduce_rows")
    return out


def permutation(seed, counter, M, device, out=None):
    """P6 epoch shuffle: i32[M] keyed bijection of [0, M) (gymrl_permutation)."""
    out = torch.empty(M, dtype=torch.int32, device=device) if out is None else out
    check(lib().gymrl_permutation(seed, counter, M, _ptr(out, torch.int32), _stream()), "gymrl_permutation")
    return out


def pack_rollout(obs, act, logp, adv, ret, packed=None):
    """P6: one 64-B record per transition (ppo_lunarlander.py:238-250).  obs [M, D]."""
    M, D = obs.shape
    packed = torch.empty(M, 16, dtype=torch.float32, device=obs.device) if packed is None else packed
    check(lib().gymrl_pack_rollout(_ptr(obs, torch.float32), _ptr(act, torch.int32), _ptr(logp, torch.float32), _ptr(adv, torch.float32),
                                   _ptr(ret, torch.float32), M, D, _ptr(packed, torch.float32), _stream()), "gymrl_pack_rollout")
    return packed


def gather_rows(src, idx, out=None):
    """gymrl_gather_rows: src[idx] for a 2-D float32 `src` whose rows are a multiple of 16 bytes (idx int32)."""
    B, D = idx.numel(), src.shape[1]
    out = torch.empty(B, D, device=src.device) if out is None else out
    check(lib().gymrl_gather_rows(_ptr(src, torch.float32), _ptr(idx, torch.int32), B, D, _ptr(out, torch.float32), _stream()), "gymrl_gather_rows")
    return out


def gather_minibatch(packed, idx, obs_dim, out=None):
    """P7: rows idx[0..B) of the packed rollout -> contiguous (obs, act, logp_old, adv, ret)."""
    B, dev = idx.numel(), packed.device
    if out is None:
        out = (torch.empty(B, obs_dim, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
               torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev))
    obs, act, logp, adv, ret = out
    check(lib().gymrl_gather_minibatch(_ptr(packed, torch.float32), _ptr(idx, torch.int32), B, obs_dim, _ptr(obs, torch.float32),
                                       _ptr(act, torch.int32), _ptr(logp, torch.float32), _ptr(adv, torch.float32), _ptr(ret, torch.float32),
                                       _stream()), "gymrl_gather_minibatch")
    return out


# -------------------------------------------------------------- optimiser ---
def sqnorm(g, out, workspace, grad_scale=1.0):
    check(lib().gymrl_sqnorm(_ptr(g, torch.float32), g.numel(), grad_scale, _ptr(out, torch.float64), _ptr(workspace), _stream()), "gymrl_sqnorm")
    return out


def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0, max_grad_norm=0.0, sqnorm_buf=None,
              clamp_abs=0.0, zero_grad=True, lr_dev=None, bias_dev=None, polyak_target=None, tau=0.0):
    """O1: Adam on one flat buffer (ppo_lunarlander.py:302-307); call sqnorm() first when clipping."""
    check(lib().gymrl_adam_step(_ptr(p, torch.float32), _ptr(g, torch.float32), _ptr(m, torch.float32), _ptr(v, torch.float32), p.numel(), lr,
                                _ptr(lr_dev, torch.float32, True), beta1, beta2, eps, step, _ptr(bias_dev, torch.float32, True), grad_scale,
                                max_grad_norm, _ptr(sqnorm_buf, torch.float64, True), clamp_abs, int(zero_grad),
                                _ptr(polyak_target, torch.float32, True), tau, _stream()), "gymrl_adam_step")


def clip_adam_step(p, g, m, v, lr, beta1, beta2, eps, step, max_grad_norm, workspace, grad_scale=1.0, sqnorm_out=None,
                   clamp_abs=0.0, zero_grad=True, lr_dev=None, bias_dev=None, polyak_target=None, tau=0.0):
    """gymrl_clip_adam_step: sqnorm() + adam_step() as two launches instead of three (same bits)."""
    check(lib().gymrl_clip_adam_step(_ptr(p, torch.float32), _ptr(g, torch.float32), _ptr(m, torch.float32), _ptr(v, torch.float32), p.numel(), lr,
                                     _ptr(lr_dev, torch.float32, True), beta1, beta2, eps, step, _ptr(bias_dev, torch.float32, True), grad_scale,
                                     max_grad_norm, _ptr(sqnorm_out, torch.float64, True), clamp_abs, int(zero_grad),
                                     _ptr(polyak_target, torch.float32, True), tau, _ptr(workspace), _stream()), "gymrl_clip_adam_step")


def adam_bias(lr, beta1, beta2, step):
    """Host arithmetic of Adam's step-dependent scalars -> 4 float32 (gymrl_adam_bias)."""
    out = (C.c_float * 4)()
    check(lib().gymrl_adam_bias(lr, beta1, beta2, step, out), "gymrl_adam_bias")
    return bytes(out)


def store_scalars(dst, payload):
    """payload: bytes (<= 3840, multiple of 4) -> device tensor `dst`, one launch."""
    if len(payload) > dst.numel() * dst.element_size():
        raise ValueError("payload larger than the destination block")
    buf = C.create_string_buffer(payload, len(payload))
    check(lib().gymrl_store_scalars(_ptr(dst), buf, len(payload), _stream()), "gymrl_store_scalars")


def soft_update(target, source, tau):
    check(lib().gymrl_soft_update(_ptr(target, torch.float32), _ptr(source, torch.float32), target.numel(), tau, _stream()), "gymrl_soft_update")


# -------------------------------------------------------------------- env ---
CARTPOLE, PENDULUM, LUNARLANDER, MOUNTAINCAR = 0, 1, 2, 3
ACROBOT = 5                    # 4 is left free for MountainCar's continuous sibling (include/gymrl.h): every entry point refuses it
ENV_KINDS = {"CartPole-v1": CARTPOLE, "Pendulum-v1": PENDULUM, "LunarLander-v3": LUNARLANDER, "MountainCar-v0": MOUNTAINCAR,
             "Acrobot-v1": ACROBOT}
# kind -> (name, observations, actions, float64 fields of a state, TimeLimit) of the classic-control envs, stated here once on
# this side of the C ABI: the episode evaluators' shape rules, start states and caps and PPO's rollout widths below read it.  The
# library's own statement is csrc/env_classic_device.hpp (ClassicDims); tests/test_episode_eval_refusals.py holds this table
# against env_dims() and against the largest cap every entry point takes.  (Not read from env_dims() here: the constants derived
# below exist at import, before the library is loaded.)
EPISODE_ENVS = {CARTPOLE: ("CartPole-v1", 4, 2, 4, 500), PENDULUM: ("Pendulum-v1", 3, 1, 2, 200),
                MOUNTAINCAR: ("MountainCar-v0", 2, 3, 2, 200), ACROBOT: ("Acrobot-v1", 6, 3, 4, 500)}
# the env kinds the DQN-family act launches step themselves (dqn_act_step, dsac_act_step: csrc/slab_step_device.hpp classic_act_tail)
FUSED_ACT_KINDS = (CARTPOLE, MOUNTAINCAR, ACROBOT)


def env_dims(kind):
    L = lib()
    return (L.gymrl_env_obs_dim(kind), L.gymrl_env_act_dim(kind), bool(L.gymrl_env_is_discrete(kind)),
            L.gymrl_env_max_steps(kind))


def env_state(kind, n, device):
    nbytes = int(lib().gymrl_env_state_bytes(kind, n))
    if nbytes == 0:
        raise RuntimeError(f"env kind {kind} unavailable")
    return torch.zeros(nbytes, dtype=torch.uint8, device=device)


def env_reset(kind, state, n, seed, env_id0, obs_out):
    check(lib().gymrl_env_reset(kind, _ptr(state), n, seed, env_id0, _ptr(obs_out, torch.float32), _stream()), "gymrl_env_reset")


def env_refill(kind, state, n, seed, env_id0, stream=None):
    st = _stream() if stream is None else _vp(stream.cuda_stream)
    check(lib().gymrl_env_refill(kind, _ptr(state), n, seed, env_id0, st), "gymrl_env_refill")


def env_step(kind, state, n, seed, env_id0, action, obs_out, rew_out, terminated_out, truncated_out,
             term_obs_out=None, done_out=None, ep_ret_out=None, ep_len_out=None, ep_stats=None):
    check(lib().gymrl_env_step(kind, _ptr(state), n, seed, env_id0, _ptr(action), _ptr(obs_out, torch.float32),
                               _ptr(term_obs_out, torch.float32, True), _ptr(rew_out, torch.float32), _ptr(terminated_out, torch.uint8),
                               _ptr(truncated_out, torch.uint8), _ptr(done_out, torch.uint8, True), _ptr(ep_ret_out, torch.float32, True),
                               _ptr(ep_len_out, torch.int32, True), _ptr(ep_stats, torch.float64, True), _stream()), "gymrl_env_step")


# ------------------------------------------------- evolution strategies ---
ES_PAIR_CHUNK = 16             # GYMRL_ES_PAIR_CHUNK: pairs per chunk of the search gradient's float64 sum (include/gymrl.h)
ES_MAX_POPULATION = 8192


def es_noise(n, k0, K, seed, generation, device, out=None):
    """eps f32[K, n] of pairs k0 .. k0 + K - 1 (include/gymrl.h: the draw map): what gymrl_es_perturb and gymrl_es_shape_grad
    draw in registers, written out for tests and tools."""
    if out is None:
        out = torch.empty(K, n, dtype=torch.float32, device=device)
    elif tuple(out.shape) != (K, n):
        raise ValueError(f"es_noise: out is {tuple(out.shape)}, {K} pairs of {n} elements need [{K}, {n}]")
    a = EsNoiseArgs()
    a.n, a.k0, a.K, a.seed, a.generation, a.out = n, k0, K, seed, generation, _ptr(out, torch.float32)
    check(lib().gymrl_es_noise(C.byref(a), _stream()), "gymrl_es_noise")
    return out


def es_stride(n):
    """The narrowest row stride the evaluators take for n parameters: n rounded up to a multiple of four floats."""
    return (n + 3) // 4 * 4


def es_perturb(theta, sigma, seed, generation, out):
    """out f32[P, stride] <- the mirrored population of the centre theta f32[n]: rows 2k / 2k + 1 = theta +- sigma * eps_k, ONE
    launch; columns n .. stride - 1 of `out` are left as they are."""
    if theta.dim() != 1 or out.dim() != 2:
        raise ValueError("es_perturb: theta is f32[n], out f32[P, stride]")
    a = EsPerturbArgs()
    a.n, a.P, a.stride, a.sigma, a.seed, a.generation = theta.numel(), out.shape[0], out.shape[1], float(sigma), seed, generation
    a.theta, a.params = _ptr(theta, torch.float32), _ptr(out, torch.float32)
    check(lib().gymrl_es_perturb(C.byref(a), _stream()), "gymrl_es_perturb")
    return out


def es_shape_grad(returns, sigma, seed, generation, grad, weights=None):
    """returns f32[P, E] of an evaluation launch -> (grad f32[n], weights f32[P]): the centred ranks of the policies' summed
    returns and the search gradient -(1 / (P sigma)) sum_k (w_2k - w_2k+1) eps_k an Adam step DESCENDS (include/gymrl.h: the
    summation order).  One launch up to 256 policies, two above."""
    if returns.dim() != 2 or grad.dim() != 1:
        raise ValueError("es_shape_grad: returns is f32[P, E], grad f32[n]")
    P, E = returns.shape
    if weights is None:
        weights = torch.empty(P, dtype=torch.float32, device=returns.device)
    elif weights.numel() != P:
        raise ValueError(f"es_shape_grad: weights has {weights.numel()} elements for {P} policies")
    a = EsShapeGradArgs()
    a.n, a.P, a.E, a.sigma, a.seed, a.generation = grad.numel(), P, E, float(sigma), seed, generation
    a.returns, a.grad, a.weights = _ptr(returns, torch.float32), _ptr(grad, torch.float32), _ptr(weights, torch.float32)
    check(lib().gymrl_es_shape_grad(C.byref(a), _stream()), "gymrl_es_shape_grad")
    return grad, weights


def snes_perturb(mu, sigma, seed, generation, out):
    """out f32[P, stride] <- the mirrored population of the centre mu f32[n] under the per-element step sizes sigma f32[n]:
    rows 2k / 2k + 1 = mu +- sigma * eps_k, ONE launch; columns n .. stride - 1 of `out` are left as they are."""
    if mu.dim() != 1 or out.dim() != 2 or tuple(sigma.shape) != tuple(mu.shape):
        raise ValueError("snes_perturb: mu and sigma are f32[n], out f32[P, stride]")
    a = SnesPerturbArgs()
    a.n, a.P, a.stride, a.seed, a.generation = mu.numel(), out.shape[0], out.shape[1], seed, generation
    a.mu, a.sigma, a.params = _ptr(mu, torch.float32), _ptr(sigma, torch.float32), _ptr(out, torch.float32)
    check(lib().gymrl_snes_perturb(C.byref(a), _stream()), "gymrl_snes_perturb")
    return out


def snes_tell(returns, mu, sigma, seed, generation, eta_mu, eta_sigma, sigma_min, sigma_max, weights=None):
    """returns [P, E] of an evaluation launch, float32 or float64 (read as it is: no cast launch) -> mu and sigma f32[n] moved
    IN PLACE by one separable-NES step on the centred ranks of the policies' summed returns (include/gymrl.h: the sums and the
    step), and weights f32[P].  One launch up to 256 policies, two above."""
    if returns.dim() != 2 or mu.dim() != 1 or tuple(sigma.shape) != tuple(mu.shape):
        raise ValueError("snes_tell: returns is [P, E], mu and sigma f32[n]")
    if returns.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"snes_tell: returns is float32 or float64, not {returns.dtype}")
    P, E = returns.shape
    if weights is None:
        weights = torch.empty(P, dtype=torch.float32, device=returns.device)
    elif weights.numel() != P:
        raise ValueError(f"snes_tell: weights has {weights.numel()} elements for {P} policies")
    a = SnesTellArgs()
    a.n, a.P, a.E, a.seed, a.generation = mu.numel(), P, E, seed, generation
    a.eta_mu, a.eta_sigma, a.sigma_min, a.sigma_max = float(eta_mu), float(eta_sigma), float(sigma_min), float(sigma_max)
    wide = returns.dtype == torch.float64
    a.returns, a.returns64 = (None, _ptr(returns)) if wide else (_ptr(returns), None)
    a.mu, a.sigma, a.weights = _ptr(mu, torch.float32), _ptr(sigma, torch.float32), _ptr(weights, torch.float32)
    check(lib().gymrl_snes_tell(C.byref(a), _stream()), "gymrl_snes_tell")
    return weights


# ------------------------------------------------------ tabular Q-learning ---
FROZENLAKE, CLIFFWALKING = 0, 1              # GYMRL_TABULAR_*
TABULAR_STATES = {FROZENLAKE: 16, CLIFFWALKING: 48}
TABULAR_ACTIONS = 4


def qlearn_state_bytes(n_runs):
    return int(lib().gymrl_qlearn_state_bytes(n_runs))


def qlearn_train(kind, Q, state, eps_table, seed, run_id0, max_episodes, max_steps, max_iters, lr, gamma, episode_rewards,
                 episode_lengths, k_out, episodes_out, is_slippery=False, shaped=False, restart=False):
    """Advance every run of Q f64[R, S, 4] by at most max_iters Q-learning steps (qlearning_frozenlake.py:96-117 /
    qlearning_cliffwalking.py:71-91, one lane per run, ONE launch); `state` (qlearn_state_bytes(R) bytes) carries the loops
    between calls, restart begins them at episode 0."""
    R = Q.shape[0]
    if tuple(Q.shape) != (R, TABULAR_STATES.get(kind, -1), TABULAR_ACTIONS):
        raise ValueError(f"Q is {tuple(Q.shape)}, env kind {kind} needs [R, {TABULAR_STATES.get(kind)}, {TABULAR_ACTIONS}]")
    if eps_table.numel() != max_episodes * max_steps or tuple(episode_rewards.shape) != (R, max_episodes) or \
            tuple(episode_lengths.shape) != (R, max_episodes) or k_out.numel() != R or episodes_out.numel() != R or \
            state.numel() < qlearn_state_bytes(R):
        raise ValueError("qlearn_train: a buffer does not have the size its run count and episode budget ask for")
    check(lib().gymrl_qlearn_train(kind, int(bool(is_slippery)), int(bool(shaped)), _ptr(Q, torch.float64), _ptr(state, torch.uint8), R,
                                   int(bool(restart)), seed, run_id0, _ptr(eps_table, torch.float64), max_episodes, max_steps, max_iters,
                                   lr, gamma, _ptr(episode_rewards, torch.float64), _ptr(episode_lengths, torch.int32),
                                   _ptr(k_out, torch.int32), _ptr(episodes_out, torch.int32), _stream()), "gymrl_qlearn_train")


def qlearn_eval(kind, Q, n_episodes, seed, stream_id0, cap, is_slippery=False):
    """n_episodes greedy episodes per run on Q f64[R, S, 4], one lane each -> (returns f64, lengths i32, reached-the-goal u8),
    each [R, n_episodes]; an episode that is not over after `cap` steps stops there with its flag 0."""
    R = Q.shape[0]
    if tuple(Q.shape) != (R, TABULAR_STATES.get(kind, -1), TABULAR_ACTIONS):
        raise ValueError(f"Q is {tuple(Q.shape)}, env kind {kind} needs [R, {TABULAR_STATES.get(kind)}, {TABULAR_ACTIONS}]")
    returns = torch.empty(R, n_episodes, dtype=torch.float64, device=Q.device)
    lengths = torch.empty(R, n_episodes, dtype=torch.int32, device=Q.device)
    flags = torch.empty(R, n_episodes, dtype=torch.uint8, device=Q.device)
    check(lib().gymrl_qlearn_eval(kind, int(bool(is_slippery)), _ptr(Q, torch.float64), R, n_episodes, seed, stream_id0, cap,
                                  _ptr(returns), _ptr(lengths), _ptr(flags), _stream()), "gymrl_qlearn_eval")
    return returns, lengths, flags


TABULAR_RULES = {"qlearning": 0, "sarsa": 1, "expected_sarsa": 2, "double_q": 3}     # GYMRL_TABULAR_RULE_*


def tabular_draws(rule, max_episodes, max_steps):
    """Draws one run can take = the entries of the epsilon table: SARSA's episode that runs out has drawn one action more."""
    return max_episodes * (max_steps + (1 if rule == TABULAR_RULES["sarsa"] else 0))


def tabular_state_bytes(rule, n_runs):
    return int(lib().gymrl_tabular_state_bytes(rule, n_runs))


def tabular_train(rule, kind, Q, state, eps_table, seed, run_id0, max_episodes, max_steps, max_iters, lr, gamma, episode_rewards,
                  episode_lengths, k_out, episodes_out, Q2=None, is_slippery=False, shaped=False, restart=False):
    """qlearn_train under one of TABULAR_RULES' values (include/gymrl.h states the loops): at most max_iters draws of every run in
    ONE launch.  Q2 f64[R, S, 4] is Double Q-learning's second table (None otherwise); eps_table has tabular_draws(...) entries;
    `state` holds tabular_state_bytes(rule, R) bytes."""
    R = Q.shape[0]
    shape = (R, TABULAR_STATES.get(kind, -1), TABULAR_ACTIONS)
    if tuple(Q.shape) != shape or (Q2 is not None and tuple(Q2.shape) != shape):
        raise ValueError(f"Q is {tuple(Q.shape)}, env kind {kind} needs [R, {TABULAR_STATES.get(kind)}, {TABULAR_ACTIONS}]")
    if rule not in TABULAR_RULES.values() or (Q2 is not None) != (rule == TABULAR_RULES["double_q"]):
        raise ValueError(f"tabular_train: rule {rule} with{'out' if Q2 is None else ''} a second table")
    if eps_table.numel() != tabular_draws(rule, max_episodes, max_steps) or tuple(episode_rewards.shape) != (R, max_episodes) or \
            tuple(episode_lengths.shape) != (R, max_episodes) or k_out.numel() != R or episodes_out.numel() != R or \
            state.numel() < tabular_state_bytes(rule, R):
        raise ValueError("tabular_train: a buffer does not have the size its rule, run count and episode budget ask for")
    a = TabularTrainArgs()
    a.rule, a.env_kind, a.is_slippery, a.shaped = rule, kind, int(bool(is_slippery)), int(bool(shaped))
    a.Q, a.state, a.n_runs, a.restart = _ptr(Q, torch.float64), _ptr(state, torch.uint8), R, int(bool(restart))
    a.seed, a.run_id0, a.eps_table, a.eps_len = seed, run_id0, _ptr(eps_table, torch.float64), eps_table.numel()
    a.max_episodes, a.max_steps, a.max_iters, a.lr, a.gamma = max_episodes, max_steps, max_iters, lr, gamma
    a.episode_rewards, a.episode_lengths = _ptr(episode_rewards, torch.float64), _ptr(episode_lengths, torch.int32)
    a.k_out, a.episodes_out = _ptr(k_out, torch.int32), _ptr(episodes_out, torch.int32)
    a.Q2 = None if Q2 is None else _ptr(Q2, torch.float64)
    check(lib().gymrl_tabular_train(C.byref(a), _stream()), "gymrl_tabular_train")


# ------------------------------------------- MountainCar-v0 rule baseline ---
MOUNTAINCAR_RULE_COEFS = (-0.09, 0.25, 0.03, 0.3, 0.9, 0.008, -0.07, 0.38, 0.07)     # mountaincar_baseline.py:37-40
MOUNTAINCAR_MAX_STEPS = EPISODE_ENVS[MOUNTAINCAR][4]


def mountaincar_rule_eval(n_episodes, seed, stream_id0, cap, device, coefs=None, start=None, want_final_state=False):
    """n_episodes episodes of MountainCar-v0 per rule policy, one lane each and ONE launch (include/gymrl.h) ->
    (returns f64, lengths i32, reached u8), each [P, n_episodes], and final_state f64[P, n_episodes, 2] when asked for.
    coefs f64[P, 9] on the device, or None: the reference's constants, P = 1.  start f64[P, n_episodes, 2] replaces the reset draws."""
    P = 1 if coefs is None else coefs.shape[0]
    if coefs is not None and tuple(coefs.shape) != (P, len(MOUNTAINCAR_RULE_COEFS)):
        raise ValueError(f"coefs is {tuple(coefs.shape)}, a population of rule policies is [P, {len(MOUNTAINCAR_RULE_COEFS)}]")
    if start is not None and tuple(start.shape) != (P, n_episodes, 2):
        raise ValueError(f"start is {tuple(start.shape)}, {P} policies x {n_episodes} episodes need [{P}, {n_episodes}, 2]")
    returns = torch.empty(P, n_episodes, dtype=torch.float64, device=device)
    lengths = torch.empty(P, n_episodes, dtype=torch.int32, device=device)
    reached = torch.empty(P, n_episodes, dtype=torch.uint8, device=device)
    final = torch.empty(P, n_episodes, 2, dtype=torch.float64, device=device) if want_final_state else None
    a = MountainCarEvalArgs()
    a.P, a.E, a.cap, a.seed, a.stream_id0 = P, n_episodes, cap, seed, stream_id0
    a.coefs, a.start = _ptr(coefs, torch.float64, True), _ptr(start, torch.float64, True)
    a.returns, a.lengths, a.reached = _ptr(returns), _ptr(lengths), _ptr(reached)
    a.final_state = _ptr(final, torch.float64, True)
    check(lib().gymrl_mountaincar_rule_eval(C.byref(a), _stream()), "gymrl_mountaincar_rule_eval")
    return (returns, lengths, reached, final) if want_final_state else (returns, lengths, reached)


# ----------------------- classic-control policies: whole episodes in one launch ---
CLASSIC_HEAD_ARGMAX, CLASSIC_HEAD_TANH = 0, 1
CLASSIC_EVAL_HEADS = {CARTPOLE: CLASSIC_HEAD_ARGMAX, PENDULUM: CLASSIC_HEAD_TANH}     # gymrl_classic_policy_eval's env kinds
MOUNTAINCAR_NET_MLP, MOUNTAINCAR_NET_DUEL_MEAN, MOUNTAINCAR_NET_DUEL_ROW = 0, 1, 2     # gymrl_mountaincar_net_eval_args.net
ACROBOT_MAX_STEPS = EPISODE_ENVS[ACROBOT][4]


def _eval_widths_ok(kind, D, A, H):
    """The layers are the env's (D, A) at a hidden width the row-slab stages carry."""
    return kind in EPISODE_ENVS and (D, A) == EPISODE_ENVS[kind][1:3] and 4 <= H <= 256 and H % 4 == 0


def classic_eval_shape_ok(kind, head, D, A, H):
    """What gymrl_classic_policy_eval takes (include/gymrl.h): CartPole-v1 under an argmax head, Pendulum-v1 under a tanh head,
    a hidden width the row-slab stages carry."""
    return kind in CLASSIC_EVAL_HEADS and CLASSIC_EVAL_HEADS[kind] == head and _eval_widths_ok(kind, D, A, H)


def classic_duel_eval_shape_ok(kind, n_hidden, D, A, H):
    """What gymrl_classic_duel_eval takes (include/gymrl.h): CartPole-v1, a trunk of one or two hidden layers, two actions, a hidden
    width the row-slab stages carry."""
    return kind == CARTPOLE and n_hidden in (1, 2) and _eval_widths_ok(kind, D, A, H)


def net_eval_shape_ok(kind, net, n_hidden, D, A, H):
    """What gymrl_mountaincar_net_eval / gymrl_acrobot_net_eval take (include/gymrl.h): a three-layer MLP (net 0: two hidden
    layers) or a dueling network (net 1: torch's mean, net 2: the DUELING epilogue's; one or two hidden layers) on the env's
    (D, A), a hidden width the row-slab stages carry."""
    return net in (0, 1, 2) and n_hidden in ((2,) if net == 0 else (1, 2)) and _eval_widths_ok(kind, D, A, H)


def mountaincar_net_eval_shape_ok(net, n_hidden, D, A, H):
    """net_eval_shape_ok on MountainCar-v0's (D, A) = (2, 3)."""
    return net_eval_shape_ok(MOUNTAINCAR, net, n_hidden, D, A, H)


def acrobot_net_eval_shape_ok(net, n_hidden, D, A, H):
    """net_eval_shape_ok on Acrobot-v1's (D, A) = (6, 3)."""
    return net_eval_shape_ok(ACROBOT, net, n_hidden, D, A, H)


def lin_fwd_image(W):
    """The forward image of a square layer's weight [H, H], H % 16 == 0 (csrc/lin_device.hpp img_fwd_index): a permutation of
    its elements, as gymrl_*_pack_images lays it out."""
    H = W.shape[0]
    if W.dim() != 2 or W.shape[1] != H or H % 16:
        raise ValueError(f"lin_fwd_image: a weight image is of a square layer with H % 16 == 0, got {tuple(W.shape)}")
    n = torch.arange(H, device=W.device).view(H, 1)
    k = torch.arange(H, device=W.device).view(1, H)
    at = (((n >> 4) * (H >> 4) + (k >> 4)) * 64 + ((k & 15) >> 2) * 16 + (n & 15)) * 4 + (k & 3)
    img = torch.empty(H * H, dtype=W.dtype, device=W.device)
    img[at.reshape(-1)] = W.detach().reshape(-1)
    return img


def _policy_addresses(who, tensors, flat, params):
    """-> (P, policy_stride, params as passed on, the tensors' device addresses in policy 0).  params = None: ONE policy, the tensors
    themselves.  params = f32[P, n]: the tensors' places in `flat`, the buffer they are views of, carried over to row 0 of the
    stack (n >= flat.numel(); rows are padded here to a multiple of four floats, the entry points' stride rule)."""
    if params is None:
        return 1, 0, None, [_ptr(t.detach(), torch.float32).value for t in tensors]
    if flat is None or params.dim() != 2 or params.shape[1] < flat.numel():
        raise ValueError(f"{who}: params is a stack [P, n] of flat buffers in the layout of `flat`")
    if params.shape[1] % 4:
        params = torch.nn.functional.pad(params, (0, 4 - params.shape[1] % 4))
    offs = [(t.data_ptr() - flat.data_ptr()) // 4 for t in tensors]
    if any(o < 0 or o + t.numel() > flat.numel() for o, t in zip(offs, tensors)):
        raise ValueError(f"{who}: the layers' tensors are not views of `flat`")
    base = _ptr(params, torch.float32).value
    return params.shape[0], params.shape[1], params, [base + 4 * o for o in offs]


def _episode_io(a, P, n_episodes, D, seed, stream_id0, start, want_final_obs, dev):
    """The starts and the outputs of an episode launch's argument block -> (returns, lengths, terminated, final_obs | None)."""
    returns = torch.empty(P, n_episodes, dtype=torch.float32, device=dev)
    lengths = torch.empty(P, n_episodes, dtype=torch.int32, device=dev)
    terminated = torch.empty(P, n_episodes, dtype=torch.uint8, device=dev)
    final = torch.empty(P, n_episodes, D, dtype=torch.float32, device=dev) if want_final_obs else None
    a.seed, a.stream_id0, a.start = seed, stream_id0, _ptr(start, torch.float64, True)
    a.returns, a.lengths, a.terminated = _ptr(returns), _ptr(lengths), _ptr(terminated)
    a.final_obs = _ptr(final, torch.float32, True)
    return returns, lengths, terminated, final


# wrapper (its entry point is gymrl_<wrapper>) -> the argument block; where the top layer (fc3 or the advantage head) goes, an index
# into w[] / b[] or the prefix of <prefix>_w / <prefix>_b; which of n_hidden / D / A the block states; whether the layers' (D, A)
# are held against the env's here (the CartPole / Pendulum entry points leave that to the library).  The trunk is w[k] / b[k] and
# the value head value_w / value_b in every block.
_EVAL_ENTRIES = {"classic_policy_eval": (ClassicEvalArgs, 2, ("D", "A"), False),
                 "classic_duel_eval": (ClassicDuelEvalArgs, "adv", ("n_hidden", "D", "A"), False),
                 "mountaincar_net_eval": (MountainCarNetEvalArgs, "head", ("n_hidden",), True),
                 "acrobot_net_eval": (AcrobotNetEvalArgs, "head", ("n_hidden",), True)}


def _episode_eval(who, kind, trunk, top, value, scalars, n_episodes, seed, stream_id0, cap, flat, params, images, start,
                  want_final_obs):
    """What the four wrappers share: the layers — (weight, bias) pairs: trunk D -> H (-> H), top H -> A, value H -> 1 or None —
    are checked, addressed (policy 0's, _policy_addresses) and written into the block _EVAL_ENTRIES[who] names next to the
    wrapper's own `scalars`, the outputs are allocated and gymrl_<who> is called -> (returns f32, lengths i32, terminated u8),
    each [P, n_episodes], and final_obs f32[P, n_episodes, D] when asked for."""
    Args, top_at, stated, env_checked = _EVAL_ENTRIES[who]
    if kind not in EPISODE_ENVS:
        raise ValueError(f"{who}: env kind {kind} has no episode evaluator")
    env, env_D, env_A, nst, _ = EPISODE_ENVS[kind]
    pairs = [tuple(pair) for pair in trunk] + [tuple(top)] + ([tuple(value)] if value is not None else [])
    if any(len(pair) != 2 or pair[0].dim() != 2 or pair[1].dim() != 1 or pair[1].shape[0] != pair[0].shape[0] for pair in pairs):
        raise ValueError(f"{who}: a layer is a (weight [N, K], bias [N]) pair")
    n, nh = len(pairs), len(trunk)
    (H, D), A = pairs[0][0].shape, top[0].shape[0]
    if nh == 2 and tuple(pairs[1][0].shape) != (H, H):
        raise ValueError(f"{who}: the trunk is not D -> H (-> H)")
    if top[0].shape[1] != H or (value is not None and tuple(value[0].shape) != (1, H)):
        raise ValueError(f"{who}: the heads are not H -> A and H -> 1")
    if env_checked and (D, A) != (env_D, env_A):
        raise ValueError(f"{who}: {env} has {env_D} observations and {env_A} actions, the layers are {D} -> .. -> {A}")
    n_pol = params.shape[0] if params is not None and params.dim() == 2 else 1
    if start is not None and tuple(start.shape) != (n_pol, n_episodes, nst):      # before any pointer is handed out
        raise ValueError(f"{who}: start is {tuple(start.shape)}, {n_pol} policies x {n_episodes} episodes need [{n_pol}, {n_episodes}, {nst}]")
    tensors = [w for w, _ in pairs] + [b for _, b in pairs]
    a = Args()
    P, stride, params, addr = _policy_addresses(who, tensors, flat, params)
    out = _episode_io(a, P, n_episodes, D, seed, stream_id0, start, want_final_obs, tensors[0].device)
    a.P, a.E, a.cap, a.H = P, n_episodes, cap, H
    for name, v in dict(scalars, **{k: v for k, v in (("n_hidden", nh), ("D", D), ("A", A)) if k in stated}).items():
        setattr(a, name, v)
    for k in range(nh):
        a.w[k], a.b[k] = addr[k], addr[n + k]
    if isinstance(top_at, int):
        a.w[top_at], a.b[top_at] = addr[nh], addr[n + nh]
    else:
        setattr(a, top_at + "_w", addr[nh])
        setattr(a, top_at + "_b", addr[n + nh])
    if value is not None:
        a.value_w, a.value_b = addr[nh + 1], addr[n + nh + 1]
    a.policy_stride, a.images = stride, _ptr(images, torch.float32, True)
    check(getattr(lib(), "gymrl_" + who)(C.byref(a), _stream()), "gymrl_" + who)
    return out if want_final_obs else out[:3]


def classic_policy_eval(kind, layers, n_episodes, seed, stream_id0, cap, head, bound=0.0, flat=None, params=None, images=None,
                        start=None, want_final_obs=False):
    """n_episodes whole episodes of CartPole-v1 / Pendulum-v1 per policy in ONE launch (include/gymrl.h
    gymrl_classic_policy_eval) -> (returns f32, lengths i32, terminated u8), each [P, n_episodes], and final_obs
    f32[P, n_episodes, D] when asked for.  layers = (fc1, fc2, fc3): Linear layers D -> H -> H -> A.  params = None: ONE policy,
    the layers' own tensors.  params = f32[P, n]: P flat parameter buffers in the layout of `flat`, the buffer the layers'
    tensors are views of (n >= flat.numel(); rows are padded here to a multiple of four floats).  Episode e of every policy starts
    from the reset draw of (seed, stream_id0 + e), or from start f64[P, n_episodes, 4 | 2]."""
    fc1, fc2, fc3 = ((m.weight, m.bias) for m in layers)
    return _episode_eval("classic_policy_eval", kind, [fc1, fc2], fc3, None, dict(env_kind=kind, head=head, bound=float(bound)),
                         n_episodes, seed, stream_id0, cap, flat, params, images, start, want_final_obs)


def classic_duel_eval(kind, trunk, value, advantage, n_episodes, seed, stream_id0, cap, flat=None, params=None, images=None,
                      start=None, want_final_obs=False):
    """classic_policy_eval for a dueling network (include/gymrl.h gymrl_classic_duel_eval): the same episodes, the same outputs.
    Every layer is a (weight, bias) tensor pair — a NoisyLinear passes its weight_mu / bias_mu as they are: trunk = one or two pairs
    (D -> H, H -> H), value = the H -> 1 head, advantage = the H -> A head.  params / flat: classic_policy_eval's offset scheme; the
    stride shifts every pointer, so whatever else lies in a row (a noisy layer's sigmas) travels unused."""
    if len(trunk) not in (1, 2):
        raise ValueError("classic_duel_eval: the trunk is one or two (weight, bias) pairs")
    return _episode_eval("classic_duel_eval", kind, trunk, advantage, value, dict(env_kind=kind), n_episodes, seed, stream_id0, cap,
                         flat, params, images, start, want_final_obs)


def _net_eval(who, kind, net, trunk, head, value, *rest):
    """mountaincar_net_eval / acrobot_net_eval: the trunk and the value head a `net` has."""
    duel = net != MOUNTAINCAR_NET_MLP
    if len(trunk) not in ((1, 2) if duel else (2,)):
        raise ValueError(f"{who}: the trunk is {'one or two' if duel else 'two'} (weight, bias) pairs")
    if duel != (value is not None):
        raise ValueError(f"{who}: a dueling network (net 1 | 2) has a value head, a three-layer one (net 0) has none")
    return _episode_eval(who, kind, trunk, head, value, dict(net=net), *rest)


def mountaincar_net_eval(net, trunk, head, n_episodes, seed, stream_id0, cap, value=None, flat=None, params=None, images=None,
                         start=None, want_final_obs=False):
    """n_episodes whole episodes of MountainCar-v0 per policy in ONE launch (include/gymrl.h gymrl_mountaincar_net_eval) ->
    (returns f32, lengths i32, terminated u8), each [P, n_episodes], and final_obs f32[P, n_episodes, 2] when asked for.  Every
    layer is a (weight, bias) tensor pair, a NoisyLinear's its weight_mu / bias_mu: trunk = the hidden layers (2 -> H, H -> H),
    head = fc3 (net 0) or the advantage head (net 1 | 2), both H -> 3, value = the H -> 1 head of a dueling network.  params /
    flat, the starts and the streams: classic_policy_eval's; start is f64[P, n_episodes, 2] = (position, velocity)."""
    return _net_eval("mountaincar_net_eval", MOUNTAINCAR, net, trunk, head, value, n_episodes, seed, stream_id0, cap, flat, params,
                     images, start, want_final_obs)


def acrobot_net_eval(net, trunk, head, n_episodes, seed, stream_id0, cap, value=None, flat=None, params=None, images=None,
                     start=None, want_final_obs=False, kind=ACROBOT):
    """mountaincar_net_eval on Acrobot-v1 (include/gymrl.h gymrl_acrobot_net_eval): the same networks (the MOUNTAINCAR_NET_*
    values of `net`), layers and outputs with trunk[0] = 6 -> H, final_obs f32[P, n_episodes, 6] and start f64[P, n_episodes, 4] =
    (th1, th2, dth1, dth2).  `kind` is what PolicyEval's call carries to tell the two entry points apart."""
    if kind != ACROBOT:
        raise ValueError(f"acrobot_net_eval: env kind {kind} is not Acrobot-v1's")
    return _net_eval("acrobot_net_eval", ACROBOT, net, trunk, head, value, n_episodes, seed, stream_id0, cap, flat, params, images,
                     start, want_final_obs)


# ---------------------- LunarLander-v3 PPO policies: whole episodes in one launch ---
LUNAR_MAX_STEPS = 1000


class LunarPolicyStack:
    """P policies of one FusedMLP's shape for lunar_policy_eval, in ONE buffer f32[P, stride]: per row every stage's packed
    weight (gymrl_mlp_pack's image) and then every stage's bias, each from a multiple of four floats on, written by ONE
    gymrl_mlp_pack_stack launch.  params f32[P, >= n]: flat parameter vectors in the layout of `flat`, the buffer the network's
    own tensors are views of; its rows may be strided (a learner's population buffer is read where it lies).  stride (floats, a
    multiple of 4): None = tight.  out: a LunarPolicyStack of the same shape from an earlier call — its buffer and descriptor
    are filled again and `out` itself is returned, nothing is allocated on the device."""

    def __new__(cls, fused, flat, params, stride=None, out=None):
        if out is None:
            return super().__new__(cls)
        if type(out) is not cls:
            raise ValueError("LunarPolicyStack: out is a LunarPolicyStack of an earlier call")
        if params.dim() == 2 and params.shape[0] != out.P:
            raise ValueError(f"LunarPolicyStack: out holds a stack of another shape ({out.P} policies, params {params.shape[0]})")
        return out                                  # __init__ runs on it with the same arguments

    def __init__(self, fused, flat, params, stride=None, out=None):
        mods = [m for m, _, _, _ in fused.stages]
        if (params.dim() != 2 or params.shape[1] < flat.numel() or params.dtype != torch.float32 or not params.is_cuda
                or (params.shape[1] > 1 and params.stride(1) != 1)):
            raise ValueError("LunarPolicyStack: params is a stack f32[P, n] of flat buffers in the layout of `flat`, on the device")
        if any(m.bias is None for m in mods):
            raise ValueError("LunarPolicyStack: every layer carries a bias")
        tensors = [m.weight for m in mods] + [m.bias for m in mods]
        offs = [(t.data_ptr() - flat.data_ptr()) // 4 for t in tensors]
        if any(o < 0 or o + t.numel() > flat.numel() for o, t in zip(offs, tensors)):
            raise ValueError("LunarPolicyStack: the layers' tensors are not views of `flat`")
        sizes = [int(lib().gymrl_mlp_packed_floats(*m.weight.shape)) for m in mods] + [(m.bias.numel() + 3) // 4 * 4 for m in mods]
        at = [sum(sizes[:k]) for k in range(len(sizes))]
        tight = sum(sizes)
        P, L = params.shape[0], len(mods)
        shape = (P, tuple(tuple(m.weight.shape) for m in mods), params.device)
        if out is not None:
            if out._shape != shape or (stride is not None and int(stride) != out.stride):
                raise ValueError("LunarPolicyStack: out holds a stack of another shape (policies, layers, stride or device)")
        else:
            self.stride = tight if stride is None else int(stride)
            if self.stride < tight or self.stride % 4:
                raise ValueError(f"LunarPolicyStack: the stride is a multiple of 4 floats and at least {tight}")
            self.P, self._shape = P, shape
            self.buffer = torch.zeros(P, self.stride, dtype=torch.float32, device=params.device)
        mlp_pack_stack(params, [(*m.weight.shape, offs[k], offs[L + k], at[k], at[L + k]) for k, m in enumerate(mods)], self.buffer)
        d = MlpDesc()
        d.n_stages = L
        base = self.buffer.data_ptr()
        for k, (m, act, src, dst) in enumerate(fused.stages):
            e = d.stage[k]
            e.W, e.b = base + 4 * at[k], base + 4 * at[L + k]
            e.out_dim, e.in_dim = m.weight.shape
            e.act, e.src, e.dst = fused._ACT[act], int(src), int(dst)
        d._keepalive = self.buffer                   # the table holds raw pointers
        self.desc = d


def _lunar_eval_args(P, n_episodes, seed, stream_id0, cap, stride, want_terminal_obs, dev):
    returns = torch.empty(P, n_episodes, dtype=torch.float64, device=dev)
    lengths = torch.empty(P, n_episodes, dtype=torch.int32, device=dev)
    terminated = torch.empty(P, n_episodes, dtype=torch.uint8, device=dev)
    final = torch.empty(P, n_episodes, 8, dtype=torch.float32, device=dev) if want_terminal_obs else None
    a = LunarEvalArgs()
    a.P, a.E, a.cap, a.seed, a.stream_id0, a.policy_stride = P, n_episodes, cap, seed, stream_id0, stride
    a.returns, a.lengths, a.terminated = _ptr(returns), _ptr(lengths), _ptr(terminated)
    a.terminal_obs = _ptr(final, torch.float32, True)
    return a, (returns, lengths, terminated, final)


def lunar_policy_eval(policy, n_episodes, seed, stream_id0, cap=LUNAR_MAX_STEPS, want_terminal_obs=True, device=None):
    """n_episodes whole LunarLander-v3 episodes per policy under the first maximum of the logits, in ONE launch (include/gymrl.h
    gymrl_lunar_policy_eval) -> (returns f64, lengths i32, terminated u8, terminal_obs f32[..., 8] | None), each [P, n_episodes].
    policy: a nn.FusedMLP (logits [4] then value [1]; P = 1, the weights as its last refresh() packed them) or a LunarPolicyStack.
    Episode e of every policy is the first episode of env stream_id0 + e under `seed`."""
    if isinstance(policy, LunarPolicyStack):
        P, stride, desc, dev = policy.P, policy.stride, policy.desc, policy.buffer.device
    else:
        dev = device if device is not None else policy.stages[0][0].weight.device
        P, stride, desc = 1, 0, policy.descriptor(16, dev)
    a, out = _lunar_eval_args(P, n_episodes, seed, stream_id0, cap, stride, want_terminal_obs, dev)
    check(lib().gymrl_lunar_policy_eval(C.byref(a), C.byref(desc), _stream()), "gymrl_lunar_policy_eval")
    return out


CLASSIC_PPO_EVAL_CAPS = {kind: EPISODE_ENVS[kind][4] for kind in (CARTPOLE, MOUNTAINCAR, ACROBOT)}       # kind -> the env's TimeLimit


def classic_ppo_eval(kind, policy, n_episodes, seed, stream_id0, cap=None, want_final_obs=False, device=None):
    """n_episodes whole CartPole-v1 / MountainCar-v0 / Acrobot-v1 episodes per policy under the first maximum of the PPO
    actor-critic's logits, in ONE launch (include/gymrl.h gymrl_classic_ppo_eval) -> (returns f64, lengths i32, terminated u8,
    final_obs f32[..., D] | None), each [P, n_episodes].  policy: a nn.FusedMLP (logits [A] then value [1]; P = 1, the weights as
    its last refresh() packed them) or a LunarPolicyStack of such networks.  cap: None = the env's TimeLimit.  Episode e of every
    policy is the first episode of env stream_id0 + e under `seed`."""
    if kind not in CLASSIC_PPO_EVAL_CAPS:
        raise ValueError(f"classic_ppo_eval: env kind {kind} is not CartPole-v1's, MountainCar-v0's or Acrobot-v1's")
    if isinstance(policy, LunarPolicyStack):
        P, stride, desc, dev = policy.P, policy.stride, policy.desc, policy.buffer.device
    else:
        dev = device if device is not None else policy.stages[0][0].weight.device
        P, stride, desc = 1, 0, policy.descriptor(16, dev)
    D = ROLLOUT_CLASSIC_DIMS[kind][0]
    n_episodes = int(n_episodes)
    returns = torch.empty(P, n_episodes, dtype=torch.float64, device=dev)
    lengths = torch.empty(P, n_episodes, dtype=torch.int32, device=dev)
    terminated = torch.empty(P, n_episodes, dtype=torch.uint8, device=dev)
    final = torch.empty(P, n_episodes, D, dtype=torch.float32, device=dev) if want_final_obs else None
    a = ClassicPpoEvalArgs()
    a.P, a.E, a.cap, a.env_kind = P, n_episodes, CLASSIC_PPO_EVAL_CAPS[kind] if cap is None else int(cap), kind
    a.seed, a.stream_id0, a.policy_stride = seed, stream_id0, stride
    a.returns, a.lengths, a.terminated = _ptr(returns), _ptr(lengths), _ptr(terminated)
    a.final_obs = _ptr(final, torch.float32, True)
    check(lib().gymrl_classic_ppo_eval(C.byref(a), C.byref(desc), _stream()), "gymrl_classic_ppo_eval")
    return returns, lengths, terminated, final


PENDULUM_MAX_STEPS = EPISODE_ENVS[PENDULUM][4]


def pendulum_ppo_eval_shape_ok(P, n_episodes, cap):
    """What gymrl_pendulum_ppo_eval takes: P >= 1 policies x E >= 1 episodes with P * E below 2^31, 1 <= cap <= 200."""
    return P >= 1 and n_episodes >= 1 and P * n_episodes <= 0x7FFFFFFF and 1 <= cap <= PENDULUM_MAX_STEPS


def pendulum_ppo_eval(policy, n_episodes, seed, stream_id0, cap=None, want_final_obs=False, device=None):
    """n_episodes whole Pendulum-v1 episodes per policy under the Gaussian actor-critic's mean (a = mu), in ONE launch
    (include/gymrl.h gymrl_pendulum_ppo_eval) -> (returns f64, lengths i32, terminated u8, final_obs f32[..., 3] | None), each
    [P, n_episodes].  policy: a nn.FusedMLP (mean [1] then value [1]; P = 1) or a LunarPolicyStack of such networks."""
    if isinstance(policy, LunarPolicyStack):
        P, stride, desc, dev = policy.P, policy.stride, policy.desc, policy.buffer.device
    else:
        dev = torch.device(device) if device is not None else policy.stages[0][0].weight.device
        P, stride = 1, 0
    n_episodes, cap = int(n_episodes), PENDULUM_MAX_STEPS if cap is None else int(cap)
    if not pendulum_ppo_eval_shape_ok(P, n_episodes, cap) or stream_id0 < 0:
        raise ValueError(f"pendulum_ppo_eval: P >= 1, episodes >= 1, 1 <= cap <= {PENDULUM_MAX_STEPS}, stream_id0 >= 0: got "
                         f"{(P, n_episodes, cap, stream_id0)}")
    if dev.type != "cuda":
        raise RuntimeError("pendulum_ppo_eval: the policy lives on the CPU; gymrl_amd ops run on the MI355X only (no CPU fallback)")
    if not isinstance(policy, LunarPolicyStack):
        desc = policy.descriptor(16, dev)
    returns = torch.empty(P, n_episodes, dtype=torch.float64, device=dev)
    lengths = torch.empty(P, n_episodes, dtype=torch.int32, device=dev)
    terminated = torch.empty(P, n_episodes, dtype=torch.uint8, device=dev)
    final = torch.empty(P, n_episodes, 3, dtype=torch.float32, device=dev) if want_final_obs else None
    a = PendulumPpoEvalArgs()
    a.P, a.E, a.cap, a.seed, a.stream_id0, a.policy_stride = P, n_episodes, cap, seed, stream_id0, stride
    a.returns, a.lengths, a.terminated = _ptr(returns), _ptr(lengths), _ptr(terminated)
    a.final_obs = _ptr(final, torch.float32, True)
    check(lib().gymrl_pendulum_ppo_eval(C.byref(a), C.byref(desc), _stream()), "gymrl_pendulum_ppo_eval")
    return returns, lengths, terminated, final


def lunar_mhc_eval(policy_desc, n_episodes, seed, stream_id0, cap=LUNAR_MAX_STEPS, want_terminal_obs=True, device=None):
    """lunar_policy_eval for PPO-full's mHC network: policy_desc is a filled _lib.MhcPolicy (its `image` as the caller left it:
    None reads the parameters in place), one policy."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    a, out = _lunar_eval_args(1, n_episodes, seed, stream_id0, cap, 0, want_terminal_obs, dev)
    check(lib().gymrl_lunar_mhc_eval(C.byref(a), C.byref(policy_desc), _stream()), "gymrl_lunar_mhc_eval")
    return out


LUNAR_NORM_STATS = 2 + 3 * 8       # RunningMeanStd.stats of the 8 observations: n, -, mean[8], S[8], std[8]


def _mlprnn_fields(P):
    """(struct, index or None, field name) of every pointer of a gymrl_mlprnn_params."""
    for name, ctype in P._fields_:
        if issubclass(ctype, C.Array):
            for i in range(ctype._length_):
                yield getattr(P, name), i, name
        else:
            yield P, None, name


class MlprnnPolicyStack:
    """P policies of one PSCN -> MLPRNN -> heads network for lunar_mlprnn_eval, in ONE buffer f32[P, stride]: row p is policy p's
    flat parameter vector.  params f32[P, n]: flat parameter vectors in the layout of `flat`, the buffer `net`'s own tensors are
    views of (the trainers' flat_params order).  stride (floats, a multiple of 4): None = n rounded up.  norm_stats f64[P, 26]
    (RunningMeanStd.stats per policy), f64[26] (one set shared by all) or None.  `desc` points at row 0.
    copy = False describes `params` in place, with no launch: f32[P, >= n] whose rows are dense, 16-byte aligned and a multiple
    of four floats apart (a learner's population buffer, es.ask()); `buffer` is then `params` itself, `desc` points into its
    rows and the stack is as current as the caller keeps that tensor."""

    def __init__(self, net, flat, params, norm_stats=None, stride=None, copy=True):
        n = flat.numel()
        tight = (n + 3) // 4 * 4
        if copy:
            if params.dim() != 2 or params.shape[1] != n or params.dtype != torch.float32 or not params.is_cuda:
                raise ValueError("MlprnnPolicyStack: params is a stack f32[P, n] of flat buffers in the layout of `flat`, on the device")
            self.stride = tight if stride is None else int(stride)
            if self.stride < tight or self.stride % 4:
                raise ValueError(f"MlprnnPolicyStack: the stride is a multiple of 4 floats and at least {tight}")
            self.P = params.shape[0]
            self.buffer = torch.zeros(self.P, self.stride, dtype=torch.float32, device=params.device)
            self.buffer[:, :n] = params
        else:
            if (params.dim() != 2 or params.shape[0] < 1 or params.shape[1] < n or params.dtype != torch.float32 or not params.is_cuda
                    or (params.shape[1] > 1 and params.stride(1) != 1)):
                raise ValueError("MlprnnPolicyStack: in place, params is f32[P, >= n] with dense rows in the layout of `flat`, "
                                 "on the device")
            self.P = params.shape[0]
            self.stride = params.stride(0) if self.P > 1 else (params.shape[1] + 3) // 4 * 4
            if self.stride < tight or self.stride % 4 or params.data_ptr() % 16 or (stride is not None and int(stride) != self.stride):
                raise ValueError(f"MlprnnPolicyStack: in place, the rows are 16-byte aligned and a multiple of 4 floats apart, at "
                                 f"least {tight}; `stride` is the tensor's own")
            self.buffer = params
        own = mlprnn_params(net)
        d = MlprnnParams()
        lo, base = flat.data_ptr(), self.buffer.data_ptr()
        for (src, i, name), (dst, _, _) in zip(_mlprnn_fields(own), _mlprnn_fields(d)):
            addr = getattr(src, name) if i is None else src[i]
            if addr is None or not lo <= addr < lo + 4 * n:
                raise ValueError("MlprnnPolicyStack: the network's tensors are not views of `flat`")
            if i is None:
                setattr(dst, name, base + (addr - lo))
            else:
                dst[i] = base + (addr - lo)
        d._keepalive, d._device = self.buffer, params.device     # the table holds raw pointers
        self.desc = d
        self.norm_stats = None
        if norm_stats is not None:
            s = torch.as_tensor(norm_stats, dtype=torch.float64).to(params.device).contiguous()
            if tuple(s.shape) not in ((LUNAR_NORM_STATS,), (self.P, LUNAR_NORM_STATS)):
                raise ValueError(f"MlprnnPolicyStack: norm_stats is f64[{LUNAR_NORM_STATS}] or f64[P, {LUNAR_NORM_STATS}]")
            self.norm_stats = s


def lunar_mlprnn_eval(policy, n_episodes, seed, stream_id0, cap=LUNAR_MAX_STEPS, norm_stats=None, want_terminal_obs=True,
                      want_h_final=False):
    """lunar_policy_eval for the recurrent PPG / PPO-RNN network (include/gymrl.h gymrl_lunar_mlprnn_eval): every episode from the
    hidden state 0, the action the first maximum of the probabilities (mlprnn_act's deterministic branch) ->
    (returns f64, lengths i32, terminated u8, terminal_obs f32[..., 8] | None[, h_final f32[..., 64]]), each [P, n_episodes].
    policy: mlprnn_params(net) (P = 1) or a MlprnnPolicyStack.  norm_stats: RunningMeanStd.stats f64[26] the network's input is
    normalised with (gymrl_running_norm_masked without update; one set for every policy), f64[P, >= 26] one per policy, or None
    — then a stack's own, and without any the network reads raw observations."""
    if isinstance(policy, MlprnnPolicyStack):
        P, stride, desc, dev = policy.P, policy.stride, policy.desc, policy.buffer.device
        if norm_stats is None:
            norm_stats = policy.norm_stats
    else:
        P, stride, desc, dev = 1, 0, policy, getattr(policy, "_device", None)
    norm_stride = 0
    if norm_stats is not None:
        _ptr(norm_stats, torch.float64)
        if norm_stats.dim() == 2 and norm_stats.shape[0] == P and norm_stats.shape[1] >= LUNAR_NORM_STATS:
            norm_stride = norm_stats.shape[1] if P > 1 else 0
        elif norm_stats.dim() != 1 or norm_stats.numel() < LUNAR_NORM_STATS:
            raise ValueError(f"norm_stats: expected f64[{LUNAR_NORM_STATS}] or f64[{P}, >= {LUNAR_NORM_STATS}], got {tuple(norm_stats.shape)}")
    if dev is None:
        dev = norm_stats.device if norm_stats is not None else torch.device("cuda", torch.cuda.current_device())
    a, out = _lunar_eval_args(P, n_episodes, seed, stream_id0, cap, stride, want_terminal_obs, dev)
    h_final = torch.empty(P, n_episodes, 64, dtype=torch.float32, device=dev) if want_h_final else None
    check(lib().gymrl_lunar_mlprnn_eval(C.byref(a), C.byref(desc), _ptr(norm_stats, torch.float64, True), norm_stride,
                                        _ptr(h_final, torch.float32, True), _stream()), "gymrl_lunar_mlprnn_eval")
    return out + (h_final,) if want_h_final else out


LUNAR_COLLECT_MAX_ENVS = 16        # gymrl_lunar_mlprnn_collect: one workgroup's rows (the statistics are sequential in env order)


def lunar_mlprnn_collect(policy, N, cap, seed, env_id0, counter0, norm_stats, reward_stats, R, gamma, out=None):
    """One collection round of the PPG-RNN / PPO-RNN trainers as ONE launch (include/gymrl.h gymrl_lunar_mlprnn_collect): N <= 16
    LunarLander-v3 episodes of envs env_id0 + i under `seed` from their reset until all have ended or `cap` steps have passed,
    sampled under the Philox counters counter0 + t.  policy: mlprnn_params(net).  norm_stats f64[26], reward_stats f64[5]
    (RunningMeanStd.stats) and R f64[N] are updated in place.  -> dict of the round's slabs in collect_round()'s layout: states
    f32[cap + 1, N, 8], act i32 / logp f32 / value f32 / live u8 [cap + 1, N], rew f32 / done u8 / dw u8 [cap, N], ep_ret f32[N],
    lengths i32[N]; rows of ended envs keep what they held (zeros in a fresh dict).  out: such a dict to write into."""
    N, cap = int(N), int(cap)
    for name, t, n in (("norm_stats", norm_stats, LUNAR_NORM_STATS), ("reward_stats", reward_stats, 5), ("R", R, N)):
        _ptr(t, torch.float64)
        if t.dim() != 1 or t.numel() != n:
            raise ValueError(f"lunar_mlprnn_collect: {name} is f64[{n}], got {tuple(t.shape)}")
    if not 1 <= N <= LUNAR_COLLECT_MAX_ENVS:
        raise ValueError(f"lunar_mlprnn_collect: 1 <= N <= {LUNAR_COLLECT_MAX_ENVS} envs (one workgroup), got {N}")
    if not 1 <= cap <= LUNAR_MAX_STEPS:
        raise ValueError(f"lunar_mlprnn_collect: 1 <= cap <= {LUNAR_MAX_STEPS}, got {cap}")
    dev = norm_stats.device
    shapes = {"states": ((cap + 1, N, 8), torch.float32), "act": ((cap + 1, N), torch.int32), "logp": ((cap + 1, N), torch.float32),
              "value": ((cap + 1, N), torch.float32), "rew": ((cap, N), torch.float32), "done": ((cap, N), torch.uint8),
              "dw": ((cap, N), torch.uint8), "live": ((cap + 1, N), torch.uint8), "ep_ret": ((N,), torch.float32),
              "lengths": ((N,), torch.int32)}
    if out is None:
        out = {k: torch.zeros(*s, dtype=dt, device=dev) for k, (s, dt) in shapes.items()}
    a = LunarCollectArgs()
    a.N, a.cap, a.seed, a.env_id0, a.counter0, a.gamma = N, cap, int(seed), int(env_id0), int(counter0), float(gamma)
    a.norm_stats, a.reward_stats, a.R = norm_stats.data_ptr(), reward_stats.data_ptr(), R.data_ptr()
    for k, (s, dt) in shapes.items():
        _need_shape(out[k], s, k)
        setattr(a, k, _ptr(out[k], dt).value)
    check(lib().gymrl_lunar_mlprnn_collect(C.byref(a), C.byref(policy), _stream()), "gymrl_lunar_mlprnn_collect")
    return out


# ============================================================== off-policy ===
def env_abandon(kind, state, n, seed, env_id0, cap, obs_inout, flag_inout=None, ep_ret_out=None, ep_len_out=None,
                ep_stats=None):
    """Start the next episode of every env whose running episode reached `cap` steps (include/gymrl.h)."""
    check(lib().gymrl_env_abandon(kind, _ptr(state), n, seed, env_id0, cap, _ptr(obs_inout, torch.float32), _ptr(flag_inout, torch.uint8, True),
                                  _ptr(ep_ret_out, torch.float32, True), _ptr(ep_len_out, torch.int32, True), _ptr(ep_stats, torch.float64, True),
                                  _stream()), "gymrl_env_abandon")


def _dev(t):
    """Pointer to a block of per-step scalars on the device (see "Per-step scalars on the device", include/gymrl.h)."""
    return _vp(None) if t is None else _ptr(t)


def replay_append(ring, cursor, src_state, src_action, src_reward, src_next_state, src_flag, cursor_dev=None):
    """D2/A3: write n rows at (cursor + i) % cap.  ring = (state, action_words, reward, next_state, flag)."""
    state, action, reward, next_state, flag = ring
    cap, D = state.shape
    AW = action.shape[1]
    n = src_reward.numel()
    check(lib().gymrl_replay_append(_ptr(state, torch.float32), _ptr(action), _ptr(reward, torch.float32), _ptr(next_state, torch.float32),
                                    _ptr(flag, torch.uint8), cap, cursor, D, AW, n, _ptr(src_state, torch.float32), _ptr(src_action),
                                    _ptr(src_reward, torch.float32), _ptr(src_next_state, torch.float32), _ptr(src_flag, torch.uint8),
                                    _dev(cursor_dev), _stream()), "gymrl_replay_append")


def replay_gather(ring, idx, action_dtype=torch.int32):
    """rows idx -> (state[B,D], action[B,AW], reward[B], next_state[B,D], flag f32[B])."""
    state, action, reward, next_state, flag = ring
    cap, D = state.shape
    AW = action.shape[1]
    B, dev = idx.numel(), state.device
    out = (torch.empty(B, D, device=dev), torch.empty(B, AW, dtype=action_dtype, device=dev),
           torch.empty(B, device=dev), torch.empty(B, D, device=dev), torch.empty(B, device=dev))
    check(lib().gymrl_replay_gather(_ptr(state, torch.float32), _ptr(action), _ptr(reward, torch.float32), _ptr(next_state, torch.float32),
                                    _ptr(flag, torch.uint8), _ptr(idx, torch.int32), B, D, AW, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(out[3]),
                                    _ptr(out[4]), _stream()), "gymrl_replay_gather")
    return out


def uniform_indices(seed, counter, size, B, device, out=None, dev=None):
    idx = torch.empty(B, dtype=torch.int32, device=device) if out is None else out
    check(lib().gymrl_uniform_indices(seed, counter, size, B, _ptr(idx), _dev(dev), _stream()), "gymrl_uniform_indices")
    return idx


def nstep_push(win, n_steps, pushes, gamma, obs, action, reward, next_obs, terminal, done, ring, cursor, dev=None,
               ep_len=None, max_episode_steps=0):
    """S2.  win = (w_state[n,N,D], w_action i32[n,N], w_reward[n,N], w_next[n,N,D], w_terminal u8, w_done u8).
    Returns True when N rows were emitted into the ring at (cursor + env) % cap."""
    w_state, w_action, w_reward, w_next, w_term, w_done = win
    state, act_w, rew, nxt, flag = ring
    N, D = obs.shape
    rc = lib().gymrl_nstep_push(_ptr(w_state, torch.float32), _ptr(w_action, torch.int32), _ptr(w_reward, torch.float32), _ptr(w_next, torch.float32),
                                _ptr(w_term, torch.uint8), _ptr(w_done, torch.uint8), n_steps, pushes, N, D, gamma, _ptr(obs, torch.float32),
                                _ptr(action, torch.int32), _ptr(reward, torch.float32), _ptr(next_obs, torch.float32),
                                _ptr(terminal, torch.uint8, True), _ptr(done, torch.uint8), _ptr(state, torch.float32), _ptr(act_w),
                                _ptr(rew, torch.float32), _ptr(nxt, torch.float32), _ptr(flag, torch.uint8), state.shape[0], cursor, _dev(dev),
                                _ptr(ep_len, torch.int32, True), max_episode_steps, _stream())
    if rc < 0:
        check(rc, "gymrl_nstep_push")
    return rc == 1


def per_workspace(B, device):
    return torch.empty(int(lib().gymrl_per_workspace_bytes(B)), dtype=torch.uint8, device=device)


def per_update(tree, cap, B, workspace, idx=None, idx_start=0, idx_is_tree=False, prio=None, prio_scalar_dev=None,
               prio_scalar=0.0, idx_start_dev=None):
    check(lib().gymrl_per_update(_ptr(tree, torch.float64), cap, _ptr(idx, torch.int32, True), idx_start, int(idx_is_tree),
                                 _ptr(prio, torch.float64, True), _ptr(prio_scalar_dev, torch.float64, True), prio_scalar, B, _dev(idx_start_dev),
                                 _ptr(workspace), _stream()), "gymrl_per_update")


def per_max_leaf(tree, cap, out, workspace):
    check(lib().gymrl_per_max_leaf(_ptr(tree, torch.float64), cap, _ptr(out, torch.float64), _ptr(workspace), _stream()), "gymrl_per_max_leaf")
    return out


def per_priorities(td, alpha, eps, clip=0.0, out=None):
    out = torch.empty(td.numel(), dtype=torch.float64, device=td.device) if out is None else out
    check(lib().gymrl_per_priorities(_ptr(td, torch.float32), td.numel(), alpha, eps, clip, _ptr(out, torch.float64), _stream()),
          "gymrl_per_priorities")
    return out


PER_TD_MAX_BATCH = 512


def per_update_td(tree, cap, idx, td, alpha, eps, workspace, clip=0.0, max_out=None, ticket=None):
    """gymrl_per_update_td: update_priorities of a sampled batch straight from the TD errors (B <= 512, cap < 2^30); with
    max_out f64[1] + ticket i32[1] (zero) the maximum over the leaves after the update comes out of the same two launches."""
    check(lib().gymrl_per_update_td(_ptr(tree, torch.float64), cap, _ptr(idx, torch.int32), _ptr(td, torch.float32), idx.numel(), alpha, eps, clip,
                                    _ptr(max_out, torch.float64, True), _ptr(ticket, torch.int32, True), _ptr(workspace), _stream()),
          "gymrl_per_update_td")


def per_sample(tree, cap, B, size, beta, workspace, u=None, seed=0, counter=0, variant_b=False, out=None, dev=None):
    if out is None:
        idx = torch.empty(B, dtype=torch.int32, device=tree.device)
        prio = torch.empty(B, dtype=torch.float64, device=tree.device)
        w = torch.empty(B, dtype=torch.float32, device=tree.device)
    else:
        idx, prio, w = out
    check(lib().gymrl_per_sample(_ptr(tree, torch.float64), cap, _ptr(u, torch.float64, True), seed, counter, B, size, beta, int(variant_b),
                                 _ptr(idx), _ptr(prio), _ptr(w), _dev(dev), _ptr(workspace), _stream()), "gymrl_per_sample")
    return idx, prio, w


def noisy_noise(nin, nout, w_eps, b_eps, eps_in=None, eps_out=None, seed=0, counter=0, counter_dev=None):
    check(lib().gymrl_noisy_noise(_ptr(eps_in, torch.float32, True), _ptr(eps_out, torch.float32, True), seed, counter, nin, nout,
                                  _ptr(w_eps, torch.float32), _ptr(b_eps, torch.float32), _dev(counter_dev), _stream()), "gymrl_noisy_noise")


def epsilon_greedy(q, epsilon, u=None, seed=0, counter=0, env_id0=0, act_out=None):
    n, A = q.shape
    act_out = torch.empty(n, dtype=torch.int32, device=q.device) if act_out is None else act_out
    check(lib().gymrl_epsilon_greedy(_ptr(q, torch.float32), _ptr(u, torch.float32, True), seed, counter, env_id0, n, A, epsilon,
                                     _ptr(act_out, torch.int32), _stream()), "gymrl_epsilon_greedy")
    return act_out


def dqn_td_loss(q, q_next_target, act, rew, flag, gamma_n, q_next_online=None, w=None, loss_sum=None):
    B, A = q.shape
    td = torch.empty(B, device=q.device)
    dq = torch.empty_like(q)
    ws = _reduce_ws(q.device) if loss_sum is not None else None
    check(lib().gymrl_dqn_td_loss(_ptr(q, torch.float32), _ptr(q_next_online, torch.float32, True), _ptr(q_next_target, torch.float32),
                                  _ptr(act, torch.int32), _ptr(rew, torch.float32), _ptr(flag, torch.float32), _ptr(w, torch.float32, True), B, A,
                                  gamma_n, _ptr(td), _ptr(dq), _ptr(loss_sum, torch.float64, True), _ptr(ws, None, True), _stream()),
          "gymrl_dqn_td_loss")
    return td, dq


C51_MAX_ACTIONS, C51_MAX_ATOMS = 8, 64          # gymrl_c51_q / gymrl_c51_loss: 1 <= A <= 8, 2 <= M <= 64


def c51_shape_ok(B, A, M, vmin, vmax):
    """What gymrl_c51_q / gymrl_c51_loss take: B >= 0 rows of 1..8 actions x 2..64 atoms on a support vmin < vmax."""
    return B >= 0 and 1 <= A <= C51_MAX_ACTIONS and 2 <= M <= C51_MAX_ATOMS and vmax > vmin and 0.0 < (vmax - vmin) / (M - 1) < 3.4e38


def _c51_rows(who, logits, A, M, vmin, vmax):
    if logits.dim() == 3 and tuple(logits.shape[1:]) == (A, M):
        logits = logits.reshape(logits.shape[0], A * M)
    if logits.dim() != 2 or logits.shape[1] != A * M or not c51_shape_ok(logits.shape[0], A, M, vmin, vmax):
        raise ValueError(f"{who}: logits are f32[B, A * M] with 1 <= A <= {C51_MAX_ACTIONS}, 2 <= M <= {C51_MAX_ATOMS} and "
                         f"vmin < vmax, not {tuple(logits.shape)} with A = {A}, M = {M}, support [{vmin}, {vmax}]")
    return logits


def c51_q(logits, A, M, vmin, vmax, argmax=False):
    """gymrl_c51_q: logits f32[B, A * M] (or [B, A, M]) of a categorical head -> q f32[B, A], the expected value of every
    action's softmax over the support z_j = vmin + j (vmax - vmin) / (M - 1); argmax=True: (q, i32[B] first maximum)."""
    logits = _c51_rows("c51_q", logits, A, M, vmin, vmax)
    _need_dev("c51_q", logits=logits)
    B = logits.shape[0]
    q = torch.empty(B, A, dtype=torch.float32, device=logits.device)
    arg = torch.empty(B, dtype=torch.int32, device=logits.device) if argmax else None
    if B == 0:                      # (an empty tensor has no data pointer to hand over; the entry point would launch nothing)
        return (q, arg) if argmax else q
    check(lib().gymrl_c51_q(_ptr(logits, torch.float32), B, A, M, vmin, vmax, _ptr(q), _ptr(arg, torch.int32, True), _stream()),
          "gymrl_c51_q")
    return (q, arg) if argmax else q


def c51_loss(logits, next_target, act, rew, flag, gamma_n, vmin, vmax, next_online=None, w=None, loss_sum=None):
    """gymrl_c51_loss: the projected cross-entropy of C51, forward and backward.  logits, next_target (and next_online: the
    double-Q selector) f32[B, A, M]; act i32[B]; rew, flag (and w: importance weights) f32[B] -> (row_loss f32[B], unweighted,
    dlogits f32[B, A, M] = d mean_b(w_b row_loss_b) / d logits, every entry written); loss_sum f64[1] += sum_b w_b row_loss_b."""
    if logits.dim() != 3 or not c51_shape_ok(*logits.shape, vmin, vmax):
        raise ValueError(f"c51_loss: logits are f32[B, A, M] with 1 <= A <= {C51_MAX_ACTIONS}, 2 <= M <= {C51_MAX_ATOMS} and "
                         f"vmin < vmax, not {tuple(logits.shape)} on the support [{vmin}, {vmax}]")
    B, A, M = logits.shape
    for name, t, shape in (("next_target", next_target, (B, A, M)), ("next_online", next_online, (B, A, M)), ("act", act, (B,)),
                           ("rew", rew, (B,)), ("flag", flag, (B,)), ("w", w, (B,)), ("loss_sum", loss_sum, (1,))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"c51_loss: {name} is {shape}, not {tuple(t.shape)}")
    _need_dev("c51_loss", logits=logits, next_target=next_target, act=act, rew=rew, flag=flag, next_online=next_online, w=w,
              loss_sum=loss_sum)
    row_loss = torch.empty(B, dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits)
    if B == 0:
        return row_loss, dlogits
    ws = _reduce_ws(logits.device) if loss_sum is not None else None
    check(lib().gymrl_c51_loss(_ptr(logits, torch.float32), _ptr(next_online, torch.float32, True), _ptr(next_target, torch.float32),
                               _ptr(act, torch.int32), _ptr(rew, torch.float32), _ptr(flag, torch.float32), _ptr(w, torch.float32, True),
                               B, A, M, vmin, vmax, gamma_n, _ptr(row_loss), _ptr(dlogits), _ptr(loss_sum, torch.float64, True),
                               _ptr(ws, None, True), _stream()), "gymrl_c51_loss")
    return row_loss, dlogits


QR_MAX_ACTIONS, QR_MAX_QUANTILES = 8, 64        # gymrl_qr_q / gymrl_qr_loss: 1 <= A <= 8, 1 <= N <= 64


def qr_shape_ok(B, A, N, kappa=1.0):
    """What gymrl_qr_q / gymrl_qr_loss take: B >= 0 rows of 1..8 actions x 1..64 quantiles, a Huber threshold that is finite and
    > 0 as a float32 (NaN compares false)."""
    return B >= 0 and 1 <= A <= QR_MAX_ACTIONS and 1 <= N <= QR_MAX_QUANTILES and 0.0 < C.c_float(kappa).value < float("inf")


def _qr_rows(who, quant, A, N):
    if quant.dim() == 3 and tuple(quant.shape[1:]) == (A, N):
        quant = quant.reshape(quant.shape[0], A * N)
    if quant.dim() != 2 or quant.shape[1] != A * N or not qr_shape_ok(quant.shape[0], A, N):
        raise ValueError(f"{who}: quant is f32[B, A * N] with 1 <= A <= {QR_MAX_ACTIONS} and 1 <= N <= {QR_MAX_QUANTILES}, "
                         f"not {tuple(quant.shape)} with A = {A}, N = {N}")
    return quant


def qr_q(quant, A, N, argmax=False):
    """gymrl_qr_q: quant f32[B, A * N] (or [B, A, N]) of a quantile head -> q f32[B, A], the mean of every action's N quantiles;
    argmax=True: (q, i32[B] first maximum)."""
    quant = _qr_rows("qr_q", quant, A, N)
    _need_dev("qr_q", quant=quant)
    B = quant.shape[0]
    q = torch.empty(B, A, dtype=torch.float32, device=quant.device)
    arg = torch.empty(B, dtype=torch.int32, device=quant.device) if argmax else None
    if B == 0:                      # (an empty tensor has no data pointer to hand over; the entry point would launch nothing)
        return (q, arg) if argmax else q
    check(lib().gymrl_qr_q(_ptr(quant, torch.float32), B, A, N, _ptr(q), _ptr(arg, torch.int32, True), _stream()), "gymrl_qr_q")
    return (q, arg) if argmax else q


def qr_loss(quant, next_target, act, rew, flag, gamma_n, kappa=1.0, next_online=None, w=None, loss_sum=None):
    """gymrl_qr_loss: the quantile-Huber loss of QR-DQN, forward and backward.  quant, next_target (and next_online: the
    double-Q selector) f32[B, A, N]; act i32[B]; rew, flag (and w: importance weights) f32[B] -> (row_loss f32[B], unweighted,
    dquant f32[B, A, N] = d mean_b(w_b row_loss_b) / d quant, every entry written); loss_sum f64[1] += sum_b w_b row_loss_b."""
    if quant.dim() != 3 or not qr_shape_ok(*quant.shape, kappa):
        raise ValueError(f"qr_loss: quant is f32[B, A, N] with 1 <= A <= {QR_MAX_ACTIONS}, 1 <= N <= {QR_MAX_QUANTILES} and a "
                         f"finite kappa > 0, not {tuple(quant.shape)} with kappa = {kappa}")
    B, A, N = quant.shape
    for name, t, shape in (("next_target", next_target, (B, A, N)), ("next_online", next_online, (B, A, N)), ("act", act, (B,)),
                           ("rew", rew, (B,)), ("flag", flag, (B,)), ("w", w, (B,)), ("loss_sum", loss_sum, (1,))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"qr_loss: {name} is {shape}, not {tuple(t.shape)}")
    _need_dev("qr_loss", quant=quant, next_target=next_target, act=act, rew=rew, flag=flag, next_online=next_online, w=w,
              loss_sum=loss_sum)
    row_loss = torch.empty(B, dtype=torch.float32, device=quant.device)
    dquant = torch.empty_like(quant)
    if B == 0:
        return row_loss, dquant
    ws = _reduce_ws(quant.device) if loss_sum is not None else None
    check(lib().gymrl_qr_loss(_ptr(quant, torch.float32), _ptr(next_online, torch.float32, True), _ptr(next_target, torch.float32),
                              _ptr(act, torch.int32), _ptr(rew, torch.float32), _ptr(flag, torch.float32), _ptr(w, torch.float32, True),
                              B, A, N, kappa, gamma_n, _ptr(row_loss), _ptr(dquant), _ptr(loss_sum, torch.float64, True),
                              _ptr(ws, None, True), _stream()), "gymrl_qr_loss")
    return row_loss, dquant


def noisy_action(mu, std, bound, eps=None, mode=0, noise_clip=0.0, seed=0, counter=0, out=None):
    """gymrl_noisy_action: Gaussian exploration noise (mode 0, numpy-float64 semantics) or TD3 target-policy
    smoothing (mode 1, torch-float32 semantics) on an action tensor; eps = explicit f64 N(0,1) draws."""
    out = torch.empty_like(mu) if out is None else out
    check(lib().gymrl_noisy_action(_ptr(mu, torch.float32), _ptr(eps, torch.float64, True), seed, counter, mu.numel(), mode, std, noise_clip, bound,
                                   _ptr(out, torch.float32), _stream()), "gymrl_noisy_action")
    return out


def mse_loss(q, y, sum_out):
    """One critic's F.mse_loss forward+backward: returns dq; sum_out (f64[1]) += sum (q - y)^2."""
    dq = torch.empty_like(q)
    check(lib().gymrl_mse_loss(_ptr(q, torch.float32), _ptr(y, torch.float32), q.numel(), _ptr(dq), _ptr(sum_out, torch.float64),
                               _ptr(_reduce_ws(q.device)), _stream()), "gymrl_mse_loss")
    return dq


def neg_mean_loss(q, sum_out):
    """Actor loss -mean(q): returns dq = -1/B; sum_out (f64[1]) += sum q."""
    dq = torch.empty_like(q)
    check(lib().gymrl_neg_mean_loss(_ptr(q, torch.float32), q.numel(), _ptr(dq), _ptr(sum_out, torch.float64), _ptr(_reduce_ws(q.device)), _stream()),
          "gymrl_neg_mean_loss")
    return dq


def dsac_target(probs_n, q1n, q2n, rew, done, log_alpha, gamma):
    y = torch.empty_like(rew)
    B, A = probs_n.shape
    check(lib().gymrl_dsac_target(_ptr(probs_n, torch.float32), _ptr(q1n, torch.float32), _ptr(q2n, torch.float32), _ptr(rew, torch.float32),
                                  _ptr(done, torch.float32), _ptr(log_alpha, torch.float32), B, A, gamma, _ptr(y), _stream()), "gymrl_dsac_target")
    return y


def dsac_critic_loss(q1, q2, act, y, sums):
    B, A = q1.shape
    d1, d2 = torch.empty_like(q1), torch.empty_like(q2)
    check(lib().gymrl_dsac_critic_loss(_ptr(q1, torch.float32), _ptr(q2, torch.float32), _ptr(act, torch.int32), _ptr(y, torch.float32), B, A,
                                       _ptr(d1), _ptr(d2), _ptr(sums, torch.float64), _ptr(_reduce_ws(q1.device)), _stream()),
          "gymrl_dsac_critic_loss")
    return d1, d2


def dsac_actor_loss(probs, q1, q2, log_alpha, sums):
    B, A = probs.shape
    dp = torch.empty_like(probs)
    check(lib().gymrl_dsac_actor_loss(_ptr(probs, torch.float32), _ptr(q1, torch.float32), _ptr(q2, torch.float32), _ptr(log_alpha, torch.float32), B,
                                      A, _ptr(dp), _ptr(sums, torch.float64), _ptr(_reduce_ws(probs.device)), _stream()), "gymrl_dsac_actor_loss")
    return dp


def dsac_alpha_step(log_alpha, m, v, sums, B, target_entropy, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, loss_out=None,
                    bias_dev=None):
    check(lib().gymrl_dsac_alpha_step(_ptr(log_alpha, torch.float32), _ptr(m, torch.float32), _ptr(v, torch.float32), _ptr(sums, torch.float64), B,
                                      target_entropy, lr, beta1, beta2, eps, step, _ptr(bias_dev, torch.float64, True),
                                      _ptr(loss_out, torch.float64, True), _stream()), "gymrl_dsac_alpha_step")


def sac_sample_fwd(mean, log_std, eps, bound):
    B, A = mean.shape
    action, logp = torch.empty_like(mean), torch.empty(B, device=mean.device)
    check(lib().gymrl_sac_sample_fwd(_ptr(mean, torch.float32), _ptr(log_std, torch.float32), _ptr(eps, torch.float32), B, A, bound, _ptr(action),
                                     _ptr(logp), _stream()), "gymrl_sac_sample_fwd")
    return action, logp


def sac_sample_bwd(mean, log_std, eps, d_action, d_logp, bound):
    B, A = mean.shape
    dm, ds = torch.empty_like(mean), torch.empty_like(mean)
    check(lib().gymrl_sac_sample_bwd(_ptr(mean, torch.float32), _ptr(log_std, torch.float32), _ptr(eps, torch.float32),
                                     _ptr(d_action, torch.float32, True), _ptr(d_logp, torch.float32, True), B, A, bound, _ptr(dm), _ptr(ds),
                                     _stream()), "gymrl_sac_sample_bwd")
    return dm, ds


def sac_target(rew, done, q1n, q2n, logp_n, log_alpha, gamma):
    y = torch.empty_like(rew)
    check(lib().gymrl_sac_target(_ptr(rew, torch.float32), _ptr(done, torch.float32), _ptr(q1n, torch.float32), _ptr(q2n, torch.float32),
                                 _ptr(logp_n, torch.float32), _ptr(log_alpha, torch.float64), rew.numel(), gamma, _ptr(y), _stream()),
          "gymrl_sac_target")
    return y


def sac_critic_loss(q1, q2, y, sums):
    d1, d2 = torch.empty_like(q1), torch.empty_like(q2)
    check(lib().gymrl_sac_critic_loss(_ptr(q1, torch.float32), _ptr(q2, torch.float32), _ptr(y, torch.float32), q1.numel(), _ptr(d1), _ptr(d2),
                                      _ptr(sums, torch.float64), _ptr(_reduce_ws(q1.device)), _stream()), "gymrl_sac_critic_loss")
    return d1, d2


def sac_actor_loss(logp, q1, q2, log_alpha, target_entropy, sums):
    dl, d1, d2 = torch.empty_like(logp), torch.empty_like(q1), torch.empty_like(q2)
    check(lib().gymrl_sac_actor_loss(_ptr(logp, torch.float32), _ptr(q1, torch.float32), _ptr(q2, torch.float32), _ptr(log_alpha, torch.float64),
                                     logp.numel(), target_entropy, _ptr(dl), _ptr(d1), _ptr(d2), _ptr(sums, torch.float64),
                                     _ptr(_reduce_ws(q1.device)), _stream()), "gymrl_sac_actor_loss")
    return dl, d1, d2


def sac_alpha_step(log_alpha, m, v, sums, B, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, loss_out=None, bias_dev=None):
    check(lib().gymrl_sac_alpha_step(_ptr(log_alpha, torch.float64), _ptr(m, torch.float64), _ptr(v, torch.float64), _ptr(sums, torch.float64), B, lr,
                                     beta1, beta2, eps, step, _ptr(bias_dev, torch.float64, True), _ptr(loss_out, torch.float64, True), _stream()),
          "gymrl_sac_alpha_step")


def running_norm(x, stats, update=True, out=None):
    N, D = x.shape
    out = torch.empty_like(x) if out is None else out
    check(lib().gymrl_running_norm(_ptr(x, torch.float32), N, D, _ptr(stats, torch.float64), int(update), _ptr(out, torch.float32), _stream()),
          "gymrl_running_norm")
    return out


def running_norm_masked(x, live, stats, update=True, out=None):
    """running_norm over the rows with live != 0 only, in row order; dead rows of `out` are left as they are."""
    N, D = x.shape
    _need_shape(live, (N,), "live")
    out = torch.empty_like(x) if out is None else out
    check(lib().gymrl_running_norm_masked(_ptr(x, torch.float32), _ptr(live, torch.uint8), N, D, _ptr(stats, torch.float64),
                                          int(update), _ptr(out, torch.float32), _stream()), "gymrl_running_norm_masked")
    return out


def reward_scaling_masked(r, live, gamma, R, stats, done=None, out=None):
    """reward_scaling over the rows with live != 0 only (R of a dead row is left as it is)."""
    _need_shape(live, (r.numel(),), "live")
    out = torch.empty_like(r) if out is None else out
    check(lib().gymrl_reward_scaling_masked(_ptr(r, torch.float32), _ptr(done, torch.uint8, True), _ptr(live, torch.uint8),
                                            r.numel(), float(gamma), _ptr(R, torch.float64), _ptr(stats, torch.float64),
                                            _ptr(out, torch.float32), _stream()), "gymrl_reward_scaling_masked")
    return out


def reward_scaling(r, done, gamma, R, stats, out=None):
    out = torch.empty_like(r) if out is None else out
    check(lib().gymrl_reward_scaling(_ptr(r, torch.float32), _ptr(done, torch.uint8, True), r.numel(), gamma, _ptr(R, torch.float64),
                                     _ptr(stats, torch.float64), _ptr(out, torch.float32), _stream()), "gymrl_reward_scaling")
    return out


# ------------------------------------------------------------ MLP forward ---
def mlp_pack(W, packed=None):
    """gymrl_mlp_pack: nn.Linear weight [out, in] -> MFMA B-operand image (f32 1-D).  Reuses `packed`."""
    out_dim, in_dim = W.shape
    n = lib().gymrl_mlp_packed_floats(out_dim, in_dim)
    if packed is None:
        packed = torch.empty(n, dtype=torch.float32, device=W.device)
    elif packed.numel() != n:
        raise ValueError("packed buffer has the wrong size")
    check(lib().gymrl_mlp_pack(_ptr(W, torch.float32), out_dim, in_dim, _ptr(packed, torch.float32), _stream()), "gymrl_mlp_pack")
    return packed


def _dense_rows(t, who, what):
    """(pointer, floats between rows) of a float32 [P, n] tensor on the device whose rows are dense (they may be strided)."""
    if t.dim() != 2 or t.shape[0] < 1:
        raise ValueError(f"{who}: {what} is f32[P, n], got {tuple(t.shape)}")
    if not t.is_cuda:
        raise RuntimeError(f"{who}: {what} lives on the MI355X: got a CPU tensor (there is no CPU fallback)")
    if t.dtype != torch.float32:
        raise TypeError(f"{who}: {what}: expected torch.float32, got {t.dtype}")
    if t.shape[1] > 1 and t.stride(1) != 1:
        raise ValueError(f"{who}: the rows of {what} must be dense")
    stride = t.stride(0) if t.shape[0] > 1 else t.shape[1]
    if stride < t.shape[1]:
        raise ValueError(f"{who}: the rows of {what} overlap")
    return t.data_ptr(), stride


def mlp_pack_stack(params, layers, packed):
    """gymrl_mlp_pack_stack (include/gymrl.h): P flat parameter vectors x len(layers) layers -> each row of `packed` in ONE launch.
    params f32[P, n] and packed f32[P, m], rows dense, possibly strided; layers: (out_dim, in_dim, w_off, b_off, w_at, b_at) per
    layer, floats into a params row (the weight [out_dim, in_dim] row-major, the bias) and into a packed row (mlp_pack's image,
    the bias padded with zeros to a multiple of four).  Floats of `packed` outside these ranges are not written.  -> packed."""
    who = "mlp_pack_stack"
    a = MlpPackStackArgs()
    a.params, a.params_stride = _dense_rows(params, who, "params")
    a.packed, a.packed_stride = _dense_rows(packed, who, "packed")
    if packed.shape[0] != params.shape[0] or packed.device != params.device:
        raise ValueError(f"{who}: packed holds {packed.shape[0]} rows on {packed.device}, params {params.shape[0]} on {params.device}")
    if not 0 < len(layers) <= MLP_MAX_STAGES:
        raise ValueError(f"{who}: 1..{MLP_MAX_STAGES} layers")
    a.P, a.n_layers = params.shape[0], len(layers)
    for e, (out_dim, in_dim, w_off, b_off, w_at, b_at) in zip(a.layer, layers):
        e.out_dim, e.in_dim, e.w_off, e.b_off, e.w_at, e.b_at = (int(v) for v in (out_dim, in_dim, w_off, b_off, w_at, b_at))
        if e.out_dim < 1 or e.in_dim < 1:
            raise ValueError(f"{who}: a layer is {e.out_dim} x {e.in_dim}")
        # the library holds the ranges to the strides; the LAST row ends with the tensor, not with the stride
        if max(e.w_off + e.out_dim * e.in_dim, e.b_off + e.out_dim) > params.shape[1]:
            raise ValueError(f"{who}: a layer's parameters end beyond a row of params ({params.shape[1]} floats)")
        if max(e.w_at + lib().gymrl_mlp_packed_floats(e.out_dim, e.in_dim), e.b_at + (e.out_dim + 3) // 4 * 4) > packed.shape[1]:
            raise ValueError(f"{who}: a layer's packed range ends beyond a row of packed ({packed.shape[1]} floats)")
    check(lib().gymrl_mlp_pack_stack(C.byref(a), _stream()), "gymrl_mlp_pack_stack")
    return packed


def mlp_desc(stages):
    """Build the stage table of gymrl_mlp_forward.  stages: list of dicts
    {W (packed by mlp_pack), shape=(out_dim, in_dim), b|None, act, src, dst, out|None}; the tensors must stay
    alive (and in place) for as long as the descriptor is used."""
    if not 0 < len(stages) <= MLP_MAX_STAGES:
        raise ValueError(f"1..{MLP_MAX_STAGES} stages")
    d = MlpDesc()
    d.n_stages = len(stages)
    for i, st in enumerate(stages):
        W, out = st["W"], st.get("out")
        e = d.stage[i]
        e.W, e.b = _ptr(W, torch.float32).value, _ptr(st.get("b"), torch.float32, True).value
        e.out_dim, e.in_dim = st["shape"]
        e.act, e.src, e.dst = int(st.get("act", ACT_NONE)), int(st["src"]), int(st["dst"])
        if e.dst < 0:
            if out is None or out.dim() != 2 or out.shape[1] != e.out_dim:
                raise ValueError("dst == -1 needs an `out` tensor [n_rows, out_dim]")
            e.out, e.out_stride = _ptr(out, torch.float32).value, out.stride(0)
    d._keepalive = list(stages)      # the table holds raw pointers: keep the tensors alive with it
    return d


def mlp_forward(x, desc):
    """gymrl_mlp_forward: the whole Linear(+Tanh|ReLU) chain on x [n_rows, in_dim] in one launch; outputs
    go to the `out` tensors named in the descriptor."""
    n, in_dim = x.shape
    check(lib().gymrl_mlp_forward(_ptr(x, torch.float32), n, in_dim, C.byref(desc), _stream()), "gymrl_mlp_forward")


# ------------------------------------------------------ MLP update passes ---
def mlp_train_workspace(C_, D, A, device):
    n = lib().gymrl_mlp_train_workspace_bytes(C_, D, A)
    return torch.empty(n, dtype=torch.uint8, device=device)


def linear_tanh_smallk(x, W, b, out):
    """out = tanh(x W^T + b) for a first layer with in_features in {2,3,4,6,8} (shared.0 + Tanh)."""
    B, D = x.shape
    check(lib().gymrl_linear_tanh_smallk(_ptr(x, torch.float32), _ptr(W, torch.float32), _ptr(b, torch.float32, True), B, D, W.shape[0],
                                         _ptr(out, torch.float32), _stream()), "gymrl_linear_tanh_smallk")
    return out


def linear_smallk(x, W, b, out):
    """out = x W^T + b for a first layer with in_features in {2,3,4,6,8} and a power-of-two width (no activation)."""
    B, D = x.shape
    check(lib().gymrl_linear_smallk(_ptr(x, torch.float32), _ptr(W, torch.float32), _ptr(b, torch.float32, True), B, D, W.shape[0],
                                    _ptr(out, torch.float32), _stream()), "gymrl_linear_smallk")
    return out


def tanh_inplace(z, bias=None):
    """z <- tanh(z + bias) in place; bias [C] broadcasts over the rows of z [..., C]."""
    check(lib().gymrl_tanh_inplace(_ptr(z, torch.float32), z.numel(), _ptr(bias, torch.float32, True), z.shape[-1], _stream()), "gymrl_tanh_inplace")
    return z


def tanh_bwd_colsum(dH, H, colsum_out, workspace):
    """dH <- dH * (1 - H^2) in place; colsum_out[c] = sum_r dH[r, c]."""
    B, Cc = dH.shape
    check(lib().gymrl_tanh_bwd_colsum(_ptr(dH, torch.float32), _ptr(H, torch.float32), B, Cc, _ptr(colsum_out, torch.float32), _ptr(workspace),
                                      _stream()), "gymrl_tanh_bwd_colsum")
    return dH


def linear_smallk_bwd(dH, H, x, dW, db, workspace, W=None, b=None):
    """First layer backward without materialising dZ: dW = (dH (1 - H^2))^T x, db = colsum.  With the layer's own
    (W, b) the kernel recomputes H = tanh(x W^T + b) instead of reading it (H may then be None).  dW = db = None: the
    block partials only (they stay in `workspace` for update_finalize)."""
    B, Cc = dH.shape
    check(lib().gymrl_linear_smallk_bwd(_ptr(dH, torch.float32), _ptr(H, torch.float32, True), _ptr(x, torch.float32), B, x.shape[1], Cc,
                                        _ptr(dW, torch.float32, True), _ptr(db, torch.float32, True), _ptr(W, torch.float32, True),
                                        _ptr(b, torch.float32, True), _ptr(workspace), _stream()), "gymrl_linear_smallk_bwd")


def heads_fwd_tanh(Zac, Wa2, ba2, Wc2, bc2, logits, value, bac=None, store_h=True):
    """Zac [B, 2C] -> tanh in place + logits [B, A] + value [B] (include/gymrl.h gymrl_heads_fwd_tanh)."""
    B, C2 = Zac.shape
    check(lib().gymrl_heads_fwd_tanh(_ptr(Zac, torch.float32), B, C2 // 2, Wa2.shape[0], _ptr(bac, torch.float32, True), _ptr(Wa2, torch.float32),
                                     _ptr(ba2, torch.float32, True), _ptr(Wc2, torch.float32), _ptr(bc2, torch.float32, True),
                                     _ptr(logits, torch.float32), _ptr(value, torch.float32), int(store_h), _stream()), "gymrl_heads_fwd_tanh")


def heads_bwd(Hac, dlogits, dv, Wa2, Wc2, dZac, dbac, dWa2, dba2, dWc2, dbc2, workspace, pre_activation=False, bac=None):
    """Backward of both heads in one pass over Hac = [Ha | Hc] (include/gymrl.h gymrl_heads_bwd)."""
    B, C2 = Hac.shape
    check(lib().gymrl_heads_bwd(_ptr(Hac, torch.float32), _ptr(dlogits, torch.float32), _ptr(dv, torch.float32), B, C2 // 2, dlogits.shape[1],
                                _ptr(Wa2, torch.float32), _ptr(Wc2, torch.float32), _ptr(dZac, torch.float32), _ptr(dbac, torch.float32),
                                _ptr(dWa2, torch.float32), _ptr(dba2, torch.float32), _ptr(dWc2, torch.float32), _ptr(dbc2, torch.float32),
                                int(pre_activation), _ptr(bac, torch.float32, True), _ptr(workspace), _stream()), "gymrl_heads_bwd")


def heads_loss_blocks(B, C_=256):
    return int(lib().gymrl_heads_loss_blocks(B, C_))


def ppo_update_shape_ok(C_, D, A):
    """gymrl_ppo_update_shape_ok: the (hidden, obs_dim, actions) the fused PPO update covers.  Host only."""
    return bool(lib().gymrl_ppo_update_shape_ok(C_, D, A))


def heads_loss_fwd_bwd(Zac, bac, Wa2, ba2, Wc2, bc2, act, logp_old, adv, ret, cfg, adv_moments, dbac, dWa2, dba2, dWc2,
                       dbc2, metric_parts, workspace):
    """Heads forward + PPO loss + heads backward in one pass; dZac overwrites Zac (include/gymrl.h).  All five gradient
    outputs None: the block partials only (they stay in `workspace` for update_finalize)."""
    B, C2 = Zac.shape
    c = PPOCfg(*[float(v) for v in cfg])
    check(lib().gymrl_heads_loss_fwd_bwd(_ptr(Zac, torch.float32), B, C2 // 2, Wa2.shape[0], _ptr(bac, torch.float32, True), _ptr(Wa2, torch.float32),
                                         _ptr(ba2, torch.float32, True), _ptr(Wc2, torch.float32), _ptr(bc2, torch.float32, True),
                                         _ptr(act, torch.int32), _ptr(logp_old, torch.float32), _ptr(adv, torch.float32), _ptr(ret, torch.float32),
                                         _ptr(adv_moments, torch.float64, True), C.byref(c), _ptr(dbac, torch.float32, True),
                                         _ptr(dWa2, torch.float32, True), _ptr(dba2, torch.float32, True), _ptr(dWc2, torch.float32, True),
                                         _ptr(dbc2, torch.float32, True), _ptr(metric_parts, torch.float64), _ptr(workspace), _stream()),
          "gymrl_heads_loss_fwd_bwd")


GAUSS_UPDATE_WIDTHS, GAUSS_UPDATE_OBS, GAUSS_UPDATE_ACT = (64, 128, 256), (2, 3, 4, 6, 8), (1,)


def ppo_gauss_update_shape_ok(C_, D, A):
    """gymrl_ppo_gauss_update_shape_ok: the (hidden, obs_dim, action components) the Gaussian head's fused PPO update covers.
    Host only."""
    for name, v in (("C", C_), ("D", D), ("A", A)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"ppo_gauss_update_shape_ok: {name} is an int, not {type(v).__name__}")
    return bool(lib().gymrl_ppo_gauss_update_shape_ok(C_, D, A))


def gauss_heads_loss_workspace(B, C_, A, device):
    """The float64 batch table of the log_std gradient, f64[ceil(B / (8 * 256 / C)), A] (gymrl_gauss_heads_loss_workspace_bytes)."""
    n = int(lib().gymrl_gauss_heads_loss_workspace_bytes(B, C_, A))
    if n <= 0:
        raise ValueError(f"gauss_heads_loss_workspace: no table for B = {B}, C = {C_}, A = {A}")
    return torch.empty(n // 8, dtype=torch.float64, device=device)


def gauss_heads_loss_fwd_bwd(Zac, bac, Wa2, ba2, Wc2, bc2, log_std, act, logp_old, adv, ret, cfg, adv_moments, dbac, dWa2, dba2,
                             dWc2, dbc2, dlog_std_out, metric_parts, workspace, dls_workspace, grid_blocks=0):
    """Heads forward + the Gaussian policy's PPO loss + heads backward in one pass; dZac overwrites Zac (include/gymrl.h
    gymrl_gauss_heads_loss_fwd_bwd).  act f32[B, A] are the minibatch's stored actions; the five head gradients and dlog_std_out
    f32[A] are written.  grid_blocks: 0 = the default grid; every output carries the same bits under every grid."""
    who = "gauss_heads_loss_fwd_bwd"
    if Zac.dim() != 2 or Zac.shape[0] < 1 or Zac.shape[1] % 2 or Zac.shape[1] // 2 not in GAUSS_UPDATE_WIDTHS:
        raise ValueError(f"{who}: Zac is f32[B >= 1, 2C] with C in {GAUSS_UPDATE_WIDTHS}, not {tuple(Zac.shape)}")
    B, Cc = Zac.shape[0], Zac.shape[1] // 2
    if Wa2.dim() != 2 or Wa2.shape[0] not in GAUSS_UPDATE_ACT or Wa2.shape[1] != Cc:
        raise ValueError(f"{who}: Wa2 is f32[A, {Cc}] with A in {GAUSS_UPDATE_ACT}, not {tuple(Wa2.shape)}")
    A = Wa2.shape[0]
    f32, f64 = torch.float32, torch.float64
    for name, t, shape, dt, opt in (
            ("Zac", Zac, (B, 2 * Cc), f32, False), ("bac", bac, (2 * Cc,), f32, True), ("Wa2", Wa2, (A, Cc), f32, False),
            ("ba2", ba2, (A,), f32, True), ("Wc2", Wc2, (1, Cc), f32, False), ("bc2", bc2, (1,), f32, True),
            ("log_std", log_std, (A,), f32, False), ("act", act, (B, A), f32, False), ("logp_old", logp_old, (B,), f32, False),
            ("adv", adv, (B,), f32, False), ("ret", ret, (B,), f32, False), ("adv_moments", adv_moments, (3,), f64, True),
            ("dbac", dbac, (2 * Cc,), f32, False), ("dWa2", dWa2, (A, Cc), f32, False), ("dba2", dba2, (A,), f32, False),
            ("dWc2", dWc2, (1, Cc), f32, False), ("dbc2", dbc2, (1,), f32, False), ("dlog_std_out", dlog_std_out, (A,), f32, False)):
        if t is None:
            if opt:
                continue
            raise ValueError(f"{who}: {name} is required")
        if tuple(t.shape) != shape and not (shape == (1, Cc) and tuple(t.shape) == (Cc,)):
            raise ValueError(f"{who}: {name} is {shape}, not {tuple(t.shape)}")
        if t.dtype != dt:
            raise ValueError(f"{who}: {name} is {dt}, not {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be contiguous")
    if metric_parts is None or metric_parts.dtype != f64 or metric_parts.dim() != 2 or metric_parts.shape[1] != 5 \
            or not metric_parts.is_contiguous():
        raise ValueError(f"{who}: metric_parts is a contiguous f64[heads_loss_blocks(B, C), 5]")
    if isinstance(grid_blocks, bool) or not isinstance(grid_blocks, int) or grid_blocks < 0:
        raise ValueError(f"{who}: grid_blocks is an int >= 0")
    if workspace is None or dls_workspace is None:
        raise ValueError(f"{who}: workspace (mlp_train_workspace) and dls_workspace (gauss_heads_loss_workspace) are required")
    if metric_parts.shape[0] < heads_loss_blocks(B, Cc):
        raise ValueError(f"{who}: metric_parts has {metric_parts.shape[0]} rows, heads_loss_blocks(B, C) = {heads_loss_blocks(B, Cc)}")
    if dls_workspace.numel() * dls_workspace.element_size() < int(lib().gymrl_gauss_heads_loss_workspace_bytes(B, Cc, A)):
        raise ValueError(f"{who}: dls_workspace is smaller than gymrl_gauss_heads_loss_workspace_bytes(B, C, A)")
    if workspace.numel() * workspace.element_size() < int(lib().gymrl_mlp_train_workspace_bytes(Cc, 0, A)):
        raise ValueError(f"{who}: workspace is smaller than gymrl_mlp_train_workspace_bytes(C, 0, A)")
    _need_dev(who, Zac=Zac, bac=bac, Wa2=Wa2, ba2=ba2, Wc2=Wc2, bc2=bc2, log_std=log_std, act=act, logp_old=logp_old, adv=adv, ret=ret,
              adv_moments=adv_moments, dbac=dbac, dWa2=dWa2, dba2=dba2, dWc2=dWc2, dbc2=dbc2, dlog_std_out=dlog_std_out,
              metric_parts=metric_parts, workspace=workspace, dls_workspace=dls_workspace)
    c = PPOCfg(*[float(v) for v in cfg])
    check(lib().gymrl_gauss_heads_loss_fwd_bwd(_ptr(Zac), B, Cc, A, _ptr(bac, None, True), _ptr(Wa2), _ptr(ba2, None, True), _ptr(Wc2),
                                               _ptr(bc2, None, True), _ptr(log_std), _ptr(act), _ptr(logp_old), _ptr(adv), _ptr(ret),
                                               _ptr(adv_moments, None, True), C.byref(c), _ptr(dbac), _ptr(dWa2), _ptr(dba2), _ptr(dWc2),
                                               _ptr(dbc2), _ptr(dlog_std_out), _ptr(metric_parts), _ptr(workspace), _ptr(dls_workspace),
                                               grid_blocks, _stream()), "gymrl_gauss_heads_loss_fwd_bwd")


# ------------------------------------------------------ update-path GEMMs ---
def gemm_workspace(device):
    return torch.empty(int(lib().gymrl_gemm_workspace_bytes()), dtype=torch.uint8, device=device)


def gemm_config(key, value):
    """Ablation variants of the hand-written GEMMs — probe build only (make -C gymrl_amd/csrc prof, GYMRL_HIP_LIB=
    .../libgymrl_hip_prof.so); the product library does not export gymrl_gemm_config."""
    L = lib()
    if not hasattr(L, "gymrl_gemm_config"):
        raise RuntimeError("gymrl_gemm_config exists in the probe build only (make -C gymrl_amd/csrc prof)")
    check(L.gymrl_gemm_config(key, value), "gymrl_gemm_config")


def linear_shape_ok(K, N):
    """Shapes gymrl_linear_fwd (x [B, K] -> [B, N]) and gymrl_linear_bwd_input (dy [B, N] -> [B, K]) cover: K in
    {64, 128} with N in {K, 2K}; K = 256 with N in {256, 512}."""
    return (K in (64, 128) and N in (K, 2 * K)) or (K == 256 and N in (256, 512))


def linear_fwd(x, W, b, out, act=True):
    """out [B, N] = tanh(x [B, K] W[N, K]^T + b) (act=False: no tanh; b None: no bias) — exact-f32 MFMA, fused epilogue."""
    B, K = x.shape
    check(lib().gymrl_linear_fwd(_ptr(x, torch.float32), _ptr(W, torch.float32), _ptr(b, torch.float32, True), B, K, W.shape[0], int(act),
                                 _ptr(out, torch.float32), _stream()), "gymrl_linear_fwd")
    return out


def linear_bwd_input(dy, W, H, dx):
    """dx [B, K] = (dy [B, N] W[N, K]) * (1 - H^2)  (H None: no factor)."""
    B, N = dy.shape
    check(lib().gymrl_linear_bwd_input(_ptr(dy, torch.float32), _ptr(W, torch.float32), _ptr(H, torch.float32, True), B, N, W.shape[1],
                                       _ptr(dx, torch.float32), _stream()), "gymrl_linear_bwd_input")
    return dx


def linear_bwd_input_add(dy, W, g, dx):
    """dx [B, 128] = g + dy [B, 256] W[256, 128]: a second Linear's input gradient added to the first one's in the epilogue."""
    B, N = dy.shape
    if g.shape != dx.shape or g.data_ptr() == dx.data_ptr():
        raise ValueError("linear_bwd_input_add: g and dx are two tensors of one shape")
    check(lib().gymrl_linear_bwd_input_add(_ptr(dy, torch.float32), _ptr(W, torch.float32), _ptr(g, torch.float32), B, N, W.shape[1],
                                           _ptr(dx, torch.float32), _stream()), "gymrl_linear_bwd_input_add")
    return dx


LINEAR_FWD, LINEAR_BWD_INPUT, LINEAR_BWD_INPUT_ADD = 0, 1, 2


def linear_geometry(kind, B, K, N):
    """(row_groups, rows_per_round) of the row-streaming kernel behind linear_fwd / linear_bwd_input / linear_bwd_input_add
    (kind LINEAR_*) at x [B, K] -> [B, N] resp. dy [B, N] -> [B, K]: a wave of the launch runs
    ceil(ceil(B / rows_per_round) / row_groups) loop iterations (include/gymrl.h gymrl_linear_geometry).  Host only."""
    g, r = C.c_int(0), C.c_int(0)
    check(lib().gymrl_linear_geometry(kind, B, K, N, C.byref(g), C.byref(r)), "gymrl_linear_geometry")
    return g.value, r.value


def linear_bwd_weight_geometry(B, N):
    s, r = C.c_int(0), C.c_int64(0)
    check(lib().gymrl_linear_bwd_weight_geometry(B, N, C.byref(s), C.byref(r)), "gymrl_linear_bwd_weight_geometry")
    return s.value, r.value


def linear_bwd_weight(dy, x, dW, workspace, db=None, partials_db=False):
    """dW [N, 256] = dy [B, N]^T x [B, 256]; db [N] = column sums of dy (None: skipped).  Overwrites.  dW = None: the slice
    partials only (they stay in `workspace` for update_finalize; partials_db: with the column-sum partials)."""
    B, N = dy.shape
    if dW is None and partials_db:
        db_arg = _ptr(workspace)                       # a non-NULL flag: nothing is written through it in this mode
    else:
        db_arg = _ptr(db, torch.float32, True)
    check(lib().gymrl_linear_bwd_weight(_ptr(dy, torch.float32), _ptr(x, torch.float32), B, N, x.shape[1], _ptr(dW, torch.float32, True), db_arg,
                                        _ptr(workspace), _stream()), "gymrl_linear_bwd_weight")
    return dW


def update_finalize(B, C_, A, D, ws_dw_ac, dWac, ws_dw_2, dW2, db2, ws_heads, dbac, dWa2, dba2, dWc2, dbc2, ws_smallk, dW1, db1):
    """gymrl_update_finalize: the second halves of a minibatch's five batch reductions (both 256-deep weight gradients, the
    heads' and the first layer's gradients) as ONE launch, from the partials their producers left in their workspaces."""
    f = lambda t: _ptr(t, torch.float32)        # noqa: E731
    check(lib().gymrl_update_finalize(B, C_, A, D, _ptr(ws_dw_ac), f(dWac), _ptr(ws_dw_2), f(dW2), f(db2), _ptr(ws_heads), f(dbac), f(dWa2), f(dba2),
                                      f(dWc2), f(dbc2), _ptr(ws_smallk), f(dW1), f(db1), _stream()), "gymrl_update_finalize")


# ------------------------------------------------------ persistent rollout ---
def rollout_lunar(env_state, n_envs, seed, env_id0, counter0, obs, act, logp, val, rew, done, ep_ret, next_value, policy_desc,
                  T, t0, nsteps, gamma, lam, noise_exp=None, gae_running=None, gae_workspace=None, ep_stats=None, wg_ticks=None,
                  refill=True, gae_carry=False):
    """gymrl_rollout_lunar: `nsteps` vector steps of collect_rollout (policy forward, draw, env step, slab writes,
    online GAE) in one launch; see include/gymrl.h for the slab layout.  gae_carry: the launch that reaches T also runs the
    blocked scan's carry pass for its envs (then gae(..., variant=3) is the apply launch alone)."""
    a = RolloutLunarArgs()
    a.env_state, a.n_envs, a.seed, a.env_id0, a.counter0 = _ptr(env_state).value, n_envs, seed, env_id0, counter0
    a.obs, a.act, a.logp = _ptr(obs, torch.float32).value, _ptr(act, torch.int32).value, _ptr(logp, torch.float32).value
    a.val, a.rew, a.done = _ptr(val, torch.float32).value, _ptr(rew, torch.float32).value, _ptr(done, torch.uint8).value
    a.ep_ret, a.next_value = _ptr(ep_ret, torch.float32, True).value, _ptr(next_value, torch.float32).value
    a.noise_exp = _ptr(noise_exp, torch.float32, True).value
    a.gae_running, a.gae_workspace = _ptr(gae_running, torch.float64, True).value, _ptr(gae_workspace, None, True).value
    a.gamma, a.lam, a.ep_stats = gamma, lam, _ptr(ep_stats, torch.float64, True).value
    a.wg_ticks = _ptr(wg_ticks, torch.int64, True).value
    a.T, a.t0, a.nsteps, a.refill = T, t0, nsteps, int(bool(refill))
    a.gae_carry = int(bool(gae_carry) and gae_running is not None)
    check(lib().gymrl_rollout_lunar(C.byref(a), C.byref(policy_desc), _stream()), "gymrl_rollout_lunar")


ROLLOUT_CLASSIC_DIMS = {kind: EPISODE_ENVS[kind][1:3] for kind in (CARTPOLE, MOUNTAINCAR, ACROBOT)}      # kind -> (observations, actions)


def _rollout_classic_args(what, kind, env_state, n_envs, seed, env_id0, counter0, obs, act, logp, val, rew, done, ep_ret, next_value, T, t0,
                          nsteps, gamma, lam, noise_exp, gae_running, gae_workspace, ep_stats):
    """The argument block of gymrl_rollout_cartpole / gymrl_rollout_classic; the slabs' shapes are checked against the kind's
    (observations, actions) before any pointer is taken."""
    if kind not in ROLLOUT_CLASSIC_DIMS:
        raise ValueError(f"{what}: env kind {kind} is not CartPole-v1's, MountainCar-v0's or Acrobot-v1's")
    D, A = ROLLOUT_CLASSIC_DIMS[kind]
    if n_envs < 1 or T < 1 or tuple(obs.shape) != (T + 1, n_envs, D):
        raise ValueError(f"{what}: obs is f32[T + 1, N, {D}] = {(T + 1, n_envs, D)}, not {tuple(obs.shape)}")
    for name, t in (("act", act), ("logp", logp), ("val", val), ("rew", rew), ("done", done), ("ep_ret", ep_ret)):
        if t is not None and tuple(t.shape) != (T, n_envs):
            raise ValueError(f"{what}: {name} is [T, N] = {(T, n_envs)}, not {tuple(t.shape)}")
    if next_value.numel() != n_envs:
        raise ValueError(f"{what}: next_value is f32[N] = {n_envs}, not {tuple(next_value.shape)}")
    if noise_exp is not None and tuple(noise_exp.shape) != (T, n_envs, A):
        raise ValueError(f"{what}: noise_exp is f32[T, N, {A}] = {(T, n_envs, A)}, not {tuple(noise_exp.shape)}")
    if gae_running is not None and tuple(gae_running.shape) != (2, n_envs):
        raise ValueError(f"{what}: gae_running is f64[2, N] = {(2, n_envs)}, not {tuple(gae_running.shape)}")
    if env_state.numel() * env_state.element_size() < int(lib().gymrl_env_state_bytes(kind, n_envs)):
        raise ValueError(f"{what}: env_state is smaller than gymrl_env_state_bytes({kind}, {n_envs})")
    a = RolloutLunarArgs()
    a.env_state, a.n_envs, a.seed, a.env_id0, a.counter0 = _ptr(env_state).value, n_envs, seed, env_id0, counter0
    a.obs, a.act, a.logp = _ptr(obs, torch.float32).value, _ptr(act, torch.int32).value, _ptr(logp, torch.float32).value
    a.val, a.rew, a.done = _ptr(val, torch.float32).value, _ptr(rew, torch.float32).value, _ptr(done, torch.uint8).value
    a.ep_ret, a.next_value = _ptr(ep_ret, torch.float32, True).value, _ptr(next_value, torch.float32).value
    a.noise_exp = _ptr(noise_exp, torch.float32, True).value
    a.gae_running, a.gae_workspace = _ptr(gae_running, torch.float64, True).value, _ptr(gae_workspace, None, True).value
    a.gamma, a.lam, a.ep_stats = gamma, lam, _ptr(ep_stats, torch.float64, True).value
    a.T, a.t0, a.nsteps = T, t0, nsteps
    return a


def rollout_cartpole(env_state, n_envs, seed, env_id0, counter0, obs, act, logp, val, rew, done, ep_ret, next_value, policy_desc,
                     T, t0, nsteps, gamma, lam, noise_exp=None, gae_running=None, gae_workspace=None, ep_stats=None):
    """gymrl_rollout_cartpole: the persistent rollout for PPO on CartPole-v1 (obs [T+1, N, 4], two actions)."""
    a = _rollout_classic_args("rollout_cartpole", CARTPOLE, env_state, n_envs, seed, env_id0, counter0, obs, act, logp, val, rew, done,
                              ep_ret, next_value, T, t0, nsteps, gamma, lam, noise_exp, gae_running, gae_workspace, ep_stats)
    check(lib().gymrl_rollout_cartpole(C.byref(a), C.byref(policy_desc), _stream()), "gymrl_rollout_cartpole")


def rollout_classic(kind, env_state, n_envs, seed, env_id0, counter0, obs, act, logp, val, rew, done, ep_ret, next_value, policy_desc,
                    T, t0, nsteps, gamma, lam, noise_exp=None, gae_running=None, gae_workspace=None, ep_stats=None):
    """gymrl_rollout_classic: the persistent rollout for PPO on CartPole-v1, MountainCar-v0 or Acrobot-v1 (obs [T+1, N, D], A
    actions: ROLLOUT_CLASSIC_DIMS[kind]); rollout_cartpole's arguments behind the env kind."""
    a = _rollout_classic_args("rollout_classic", kind, env_state, n_envs, seed, env_id0, counter0, obs, act, logp, val, rew, done,
                              ep_ret, next_value, T, t0, nsteps, gamma, lam, noise_exp, gae_running, gae_workspace, ep_stats)
    check(lib().gymrl_rollout_classic(kind, C.byref(a), C.byref(policy_desc), _stream()), "gymrl_rollout_classic")


def rollout_pendulum_shape_ok(n_envs, T, t0, nsteps):
    """What gymrl_rollout_pendulum takes: N >= 1 envs, T >= 1 and a step window inside [0, T]."""
    return n_envs >= 1 and T >= 1 and t0 >= 0 and nsteps >= 0 and t0 + nsteps <= T


def rollout_pendulum(env_state, n_envs, seed, env_id0, counter0, obs, act, logp, val, rew, done, ep_ret, next_value, policy_desc,
                     log_std, T, t0, nsteps, gamma, lam, reward_scale=1.0, noise_normal=None, gae_running=None, gae_workspace=None,
                     ep_stats=None):
    """gymrl_rollout_pendulum: the persistent rollout for PPO on Pendulum-v1 under the Gaussian policy (obs [T+1, N, 3], act
    f32[T, N] the unclipped draw, log_std f32[1], noise_normal f32[T, N, 1]); rew holds reward * reward_scale."""
    what = "rollout_pendulum"
    if not rollout_pendulum_shape_ok(n_envs, T, t0, nsteps):
        raise ValueError(f"{what}: N >= 1, T >= 1 and 0 <= t0 <= t0 + nsteps <= T, got {(n_envs, T, t0, nsteps)}")
    if tuple(obs.shape) != (T + 1, n_envs, 3):
        raise ValueError(f"{what}: obs is f32[T + 1, N, 3] = {(T + 1, n_envs, 3)}, not {tuple(obs.shape)}")
    for name, t in (("act", act), ("logp", logp), ("val", val), ("rew", rew), ("done", done), ("ep_ret", ep_ret)):
        if t is not None and tuple(t.shape) != (T, n_envs):
            raise ValueError(f"{what}: {name} is [T, N] = {(T, n_envs)}, not {tuple(t.shape)}")
    if next_value.numel() != n_envs:
        raise ValueError(f"{what}: next_value is f32[N] = {n_envs}, not {tuple(next_value.shape)}")
    if tuple(log_std.shape) != (1,):
        raise ValueError(f"{what}: log_std is f32[1], not {tuple(log_std.shape)}")
    if noise_normal is not None and tuple(noise_normal.shape) != (T, n_envs, 1):
        raise ValueError(f"{what}: noise_normal is f32[T, N, 1] = {(T, n_envs, 1)}, not {tuple(noise_normal.shape)}")
    if gae_running is not None and (tuple(gae_running.shape) != (2, n_envs) or gae_workspace is None):
        raise ValueError(f"{what}: gae_running is f64[2, N] = {(2, n_envs)} and comes with gae_workspace")
    _need_dev(what, env_state=env_state, obs=obs, act=act, logp=logp, val=val, rew=rew, done=done, ep_ret=ep_ret, next_value=next_value,
              log_std=log_std, noise_normal=noise_normal, gae_running=gae_running, gae_workspace=gae_workspace, ep_stats=ep_stats)
    if env_state.numel() * env_state.element_size() < int(lib().gymrl_env_state_bytes(PENDULUM, n_envs)):
        raise ValueError(f"{what}: env_state is smaller than gymrl_env_state_bytes({PENDULUM}, {n_envs})")
    a = RolloutPendulumArgs()
    a.env_state, a.n_envs, a.seed, a.env_id0, a.counter0 = _ptr(env_state).value, n_envs, seed, env_id0, counter0
    a.obs, a.act, a.logp = _ptr(obs, torch.float32).value, _ptr(act, torch.float32).value, _ptr(logp, torch.float32).value
    a.val, a.rew, a.done = _ptr(val, torch.float32).value, _ptr(rew, torch.float32).value, _ptr(done, torch.uint8).value
    a.ep_ret, a.next_value = _ptr(ep_ret, torch.float32, True).value, _ptr(next_value, torch.float32).value
    a.log_std, a.noise_normal = _ptr(log_std, torch.float32).value, _ptr(noise_normal, torch.float32, True).value
    a.reward_scale = float(reward_scale)
    a.gae_running, a.gae_workspace = _ptr(gae_running, torch.float64, True).value, _ptr(gae_workspace, None, True).value
    a.gamma, a.lam, a.ep_stats = gamma, lam, _ptr(ep_stats, torch.float64, True).value
    a.T, a.t0, a.nsteps = T, t0, nsteps
    check(lib().gymrl_rollout_pendulum(C.byref(a), C.byref(policy_desc), _stream()), "gymrl_rollout_pendulum")


def rollout_lunar_mhc(env_state, n_envs, seed, env_id0, counter0, obs, act, logp, val, rew, done, ep_ret, next_value, policy_desc,
                      T, t0, nsteps, gamma, lam, ent=None, lam2=0.0, noise_exp=None, gae_running=None, gae_running2=None,
                      gae_workspace=None, ep_stats=None, refill=True):
    """gymrl_rollout_lunar_mhc: the persistent LunarLander rollout with PPO-full's mHC network (a filled _lib.MhcPolicy) as the
    policy; `ent` [T, N] receives the behaviour entropies, gae_running2 / lam2 switch the decoupled-lambda maps on."""
    a = RolloutLunarArgs()
    a.env_state, a.n_envs, a.seed, a.env_id0, a.counter0 = _ptr(env_state).value, n_envs, seed, env_id0, counter0
    a.obs, a.act, a.logp = _ptr(obs, torch.float32).value, _ptr(act, torch.int32).value, _ptr(logp, torch.float32).value
    a.val, a.rew, a.done = _ptr(val, torch.float32).value, _ptr(rew, torch.float32).value, _ptr(done, torch.uint8).value
    a.ep_ret, a.next_value = _ptr(ep_ret, torch.float32, True).value, _ptr(next_value, torch.float32).value
    a.noise_exp = _ptr(noise_exp, torch.float32, True).value
    a.gae_running, a.gae_workspace = _ptr(gae_running, torch.float64, True).value, _ptr(gae_workspace, None, True).value
    a.gae_running2, a.lam2, a.ent = _ptr(gae_running2, torch.float64, True).value, lam2, _ptr(ent, torch.float32, True).value
    a.gamma, a.lam, a.ep_stats = gamma, lam, _ptr(ep_stats, torch.float64, True).value
    a.T, a.t0, a.nsteps, a.refill = T, t0, nsteps, int(bool(refill))
    check(lib().gymrl_rollout_lunar_mhc(C.byref(a), C.byref(policy_desc), _stream()), "gymrl_rollout_lunar_mhc")


# ------------------------------------------------ low-latency Linear layers --
LIN_ACT = {None: 0, "none": 0, "tanh": 1, "relu": 2, "clamp": 3, "dueling": 4, "silu": 5}
LIN_MAX_ITEMS = 4


def _rows(t, allow_none=False):
    """(pointer, row stride) of a 2-D f32 device tensor whose rows are contiguous (column slices are fine)."""
    if t is None:
        if allow_none:
            return None, 0
        raise ValueError("tensor required")
    if not t.is_cuda:
        raise RuntimeError("gymrl_amd ops run on the MI355X only: got a CPU tensor (there is no CPU fallback)")
    if t.dtype != torch.float32 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError("expected a 2-D float32 tensor with contiguous rows")
    return t.data_ptr(), (t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1]))


def _as_items(v, n):
    if isinstance(v, (list, tuple)):
        if len(v) != n:
            raise ValueError("every per-item argument needs the same number of items")
        return list(v)
    return [v] * n


def _lin_pack(n, **cols):
    """Build the gymrl_lin_item array; cols: field -> list of (ptr | None).  Returns the ctypes array."""
    from ._lib import LinItem
    arr = (LinItem * n)()
    for f, vals in cols.items():
        for i, v in enumerate(vals):
            setattr(arr[i], f, v)
    return arr


def _same(vals, what):
    if any(v != vals[0] for v in vals):
        raise ValueError(f"items of one launch must share {what}")
    return vals[0]


def lin_workspace(B, N, K, n_items, device):
    n = lib().gymrl_lin_workspace_bytes(B, N, K, n_items)
    return torch.empty(max(n // 4, 1), dtype=torch.float32, device=device) if n else None


def lin_fwd(x, w, b, act=0, x2=None, out=None, lo=0.0, hi=0.0, argmax=None):
    """gymrl_lin_fwd: y = act(cat(x, x2) w^T + b) in one launch.  Every tensor argument may be a list (<= 4 layers of one
    shape in the same launch: twin critics, two heads on one input); returns y or the list of ys."""
    multi = isinstance(w, (list, tuple))
    n = len(w) if multi else 1
    xs, x2s, ws, bs = _as_items(x, n), _as_items(x2, n), _as_items(w, n), _as_items(b, n)
    B = xs[0].shape[0]
    N, K = ws[0].shape
    K1 = xs[0].shape[1]
    acts = _as_items(act, n)
    outs = _as_items(out, n) if out is not None else [torch.empty(B, N - 1 if a == 4 else N, dtype=torch.float32,
                                                                  device=xs[0].device) for a in acts]
    px, ldx = zip(*(_rows(t) for t in xs))
    px2, ldx2 = zip(*(_rows(t, True) for t in x2s))
    py, ldy = zip(*(_rows(t) for t in outs))
    for wt, xt, x2t in zip(ws, xs, x2s):
        if tuple(wt.shape) != (N, K) or xt.shape != (B, K1) or K1 + (0 if x2t is None else x2t.shape[1]) != K:
            raise ValueError("lin_fwd: shape mismatch between the items of one launch")
    items = _lin_pack(n, x=px, x2=px2, w=[_ptr(t, torch.float32).value for t in ws],
                      b=[None if t is None else _ptr(t, torch.float32).value for t in bs], y=py,
                      act=acts, lo=_as_items(lo, n), hi=_as_items(hi, n),
                      argmax=[None if t is None else _ptr(t, torch.int32).value for t in _as_items(argmax, n)])
    check(lib().gymrl_lin_fwd(items, n, B, K, K1, N, _same(ldx, "a row stride"), _same(ldx2, "a row stride"), _same(ldy, "a row stride"), _stream()),
          "gymrl_lin_fwd")
    return outs if multi else outs[0]


def lin_bwd_input(dy, y, w, act=0, K1=None, dx=None, dx2=None, want=(True, True), lo=0.0, hi=0.0, accumulate=False,
                  sum_items=False):
    """gymrl_lin_bwd_input: (dx | dx2) = (dy * act'(y)) w.  K1 = columns of the first input block (None: all of K);
    want = which of the two blocks to compute.  Lists batch up to 4 layers; sum_items: the layers share their input and
    ONE gradient (the sum) is returned.  Returns (dx, dx2) (None where skipped)."""
    multi = isinstance(w, (list, tuple))
    n = len(w) if multi else 1
    dys, ys, ws = _as_items(dy, n), _as_items(y, n), _as_items(w, n)
    B, N = dys[0].shape
    K = ws[0].shape[1]
    K1 = K if K1 is None else K1
    dev = dys[0].device
    want1, want2 = want[0] and K1 > 0, want[1] and K1 < K
    n_out = 1 if sum_items else n
    dxs = _as_items(dx, n) if dx is not None else [torch.empty(B, K1, dtype=torch.float32, device=dev)
                                                   if want1 and i < n_out else None for i in range(n)]
    dx2s = _as_items(dx2, n) if dx2 is not None else [torch.empty(B, K - K1, dtype=torch.float32, device=dev)
                                                      if want2 and i < n_out else None for i in range(n)]
    if sum_items:                       # the C side reads item 0's destinations only; keep the strides uniform
        dxs, dx2s = [dxs[0]] * n, [dx2s[0]] * n
    pdy, ldy = zip(*(_rows(t) for t in dys))
    acts = _as_items(act, n)
    py, ldyy = zip(*(_rows(t, a == 0) for t, a in zip(ys, acts)))
    if any(a != 0 and l1 != l2 for a, l1, l2 in zip(acts, ldyy, ldy)):
        raise ValueError("lin_bwd_input: dy and y need the same row stride")
    pdx, lddx = zip(*(_rows(t, True) for t in dxs))
    pdx2, lddx2 = zip(*(_rows(t, True) for t in dx2s))
    items = _lin_pack(n, dy=pdy, y=py, w=[_ptr(t, torch.float32).value for t in ws], dx=pdx, dx2=pdx2,
                      act=acts, lo=_as_items(lo, n), hi=_as_items(hi, n))
    check(lib().gymrl_lin_bwd_input(items, n, B, N, K, K1, _same(ldy, "a row stride"), _same(lddx, "a row stride"), _same(lddx2, "a row stride"),
                                    int(accumulate), int(sum_items), _stream()), "gymrl_lin_bwd_input")
    if sum_items:
        return dxs[0], dx2s[0]
    return (dxs, dx2s) if multi else (dxs[0], dx2s[0])


def lin_bwd_weight(dy, y, x, dw, db=None, act=0, x2=None, lo=0.0, hi=0.0, accumulate=False, workspace=None):
    """gymrl_lin_bwd_weight: dw (+)= (dy * act'(y))^T cat(x, x2), db (+)= its column sums, written straight into dw / db
    (e.g. the views of a flat gradient buffer).  Lists batch up to 4 layers."""
    multi = isinstance(dw, (list, tuple))
    n = len(dw) if multi else 1
    dys, ys, xs, x2s, dws, dbs = (_as_items(v, n) for v in (dy, y, x, x2, dw, db))
    B, N = dys[0].shape
    K1 = xs[0].shape[1]
    K = dws[0].shape[1]
    pdy, ldy = zip(*(_rows(t) for t in dys))
    acts = _as_items(act, n)
    py, ldyy = zip(*(_rows(t, a == 0) for t, a in zip(ys, acts)))
    if any(a != 0 and l1 != l2 for a, l1, l2 in zip(acts, ldyy, ldy)):
        raise ValueError("lin_bwd_weight: dy and y need the same row stride")
    px, ldx = zip(*(_rows(t) for t in xs))
    px2, ldx2 = zip(*(_rows(t, True) for t in x2s))
    if workspace is None and B > 512:
        workspace = lin_workspace(B, N, K, n, dys[0].device)
    items = _lin_pack(n, dy=pdy, y=py, x=px, x2=px2, dw=[_ptr(t, torch.float32).value for t in dws],
                      db=[None if t is None else _ptr(t, torch.float32).value for t in dbs],
                      act=acts, lo=_as_items(lo, n), hi=_as_items(hi, n))
    check(lib().gymrl_lin_bwd_weight(items, n, B, N, K, K1, _same(ldy, "a row stride"), _same(ldx, "a row stride"), _same(ldx2, "a row stride"),
                                     int(accumulate), _ptr(workspace, torch.float32, True), _stream()), "gymrl_lin_bwd_weight")
    return dw


def _noisy_layers(layers):
    """layers: list of dicts with w_mu, w_sigma, w_eps, b_mu, b_sigma, b_eps (+ optional w_eps_copy, b_eps_copy, dw_mu,
    dw_sigma, db_mu, db_sigma) tensors -> (ctypes array, K, total rows)."""
    from ._lib import NoisyLayer
    arr = (NoisyLayer * len(layers))()
    K = layers[0]["w_mu"].shape[1]
    rows = 0
    for i, L in enumerate(layers):
        if L["w_mu"].shape[1] != K:
            raise ValueError("noisy layers of one launch share their input width")
        for f, ct in NoisyLayer._fields_:
            if ct is C.c_void_p and f != "counter_dev":
                t = L.get(f)
                setattr(arr[i], f, None if t is None else _ptr(t, torch.float32).value)
        arr[i].seed, arr[i].counter, arr[i].draw = int(L.get("seed", 0)), int(L.get("counter", 0)), int(bool(L.get("draw")))
        arr[i].eval = int(bool(L.get("eval")))
        cd = L.get("counter_dev")
        arr[i].counter_dev = None if cd is None else _ptr(cd).value
        arr[i].n_out = L["w_mu"].shape[0]
        rows += L["w_mu"].shape[0]
    return arr, K, rows


def noisy_combine(layers, training=True, images=None):
    """gymrl_noisy_combine: stacked effective parameters (W [rows, K], b [rows]) of NoisyLinear layers in one launch.
    images: [(W [H, H], img_fwd or None, img_bwd or None)] — gymrl_noisy_combine_images: the MFMA-operand images of square
    weights rebuilt on extra workgroups of the same launch (flat f32[H * H] outputs)."""
    arr, K, rows = _noisy_layers(layers)
    dev = layers[0]["w_mu"].device
    W, b = torch.empty(rows, K, dtype=torch.float32, device=dev), torch.empty(rows, dtype=torch.float32, device=dev)
    if images:
        from ._lib import WeightImage
        ims = (WeightImage * len(images))()
        for i, (w, f, bw) in enumerate(images):
            H = w.shape[0]
            if w.shape != (H, H) or not w.is_contiguous() or any(t is not None and t.numel() != H * H for t in (f, bw)):
                raise ValueError("noisy_combine: an image needs a contiguous square weight and H * H floats per image")
            ims[i].W, ims[i].H = _ptr(w, torch.float32).value, H
            ims[i].img_fwd, ims[i].img_bwd = (None if t is None else _ptr(t, torch.float32).value for t in (f, bw))
        check(lib().gymrl_noisy_combine_images(arr, len(layers), K, int(training), _ptr(W), _ptr(b), ims, len(images), _stream()),
              "gymrl_noisy_combine_images")
        return W, b
    check(lib().gymrl_noisy_combine(arr, len(layers), K, int(training), _ptr(W), _ptr(b), _stream()), "gymrl_noisy_combine")
    return W, b


def noisy_split(layers, dW, db, training=True, accumulate=False):
    """gymrl_noisy_split: the stacked gradient back to every layer's dw_mu / dw_sigma / db_mu / db_sigma tensors."""
    arr, K, rows = _noisy_layers(layers)
    if tuple(dW.shape) != (rows, K):
        raise ValueError("noisy_split: stacked gradient shape mismatch")
    check(lib().gymrl_noisy_split(arr, len(layers), K, int(training), _ptr(dW, torch.float32), _ptr(db, torch.float32), int(accumulate), _stream()),
          "gymrl_noisy_split")


def dueling_bwd(dq):
    """gymrl_dueling_bwd: dq [B, A] -> dS [B, A + 1] (advantage columns, then the value column)."""
    B, A = dq.shape
    dS = torch.empty(B, A + 1, dtype=torch.float32, device=dq.device)
    check(lib().gymrl_dueling_bwd(_ptr(dq, torch.float32), B, A, _ptr(dS), _stream()), "gymrl_dueling_bwd")
    return dS



# ------------------------------------------------ mHC backbone (inference) --
def mhc_gates(h, norm_w, w, alpha, beta, sk_it, stats=False):
    """gymrl_mhc_gates: h [B, n, D] -> (pre [B, n], post [B, n], mix [B, n, n], read [B, D]); stats=True appends the per-row
    read-out sums f32[B, n*n + 2n + 1] gymrl_mhc_gates_bwd takes (n = 2, n*D in (256, 512))."""
    B, n, D = h.shape
    dev = h.device
    pre, post = torch.empty(B, n, device=dev), torch.empty(B, n, device=dev)
    mix, read = torch.empty(B, n, n, device=dev), torch.empty(B, D, device=dev)
    st = torch.empty(B, n * n + 2 * n + 1, device=dev) if stats else None
    check(lib().gymrl_mhc_gates(_ptr(h, torch.float32), _ptr(norm_w, torch.float32), _ptr(w, torch.float32), _ptr(alpha, torch.float32),
                                _ptr(beta, torch.float32), B, n, D, sk_it, _ptr(pre), _ptr(post), _ptr(mix), _ptr(read),
                                None if st is None else _ptr(st), _stream()), "gymrl_mhc_gates")
    return (pre, post, mix, read, st) if stats else (pre, post, mix, read)


def mhc_combine(post, mix, out, h, act=0):
    """gymrl_mhc_combine: h'[b, i] = post[b, i] act(out[b]) + sum_j mix[b, i, j] h[b, j]; act = 0 or LIN_ACT["silu"]."""
    B, n, D = h.shape
    h_out = torch.empty_like(h)
    check(lib().gymrl_mhc_combine(_ptr(post, torch.float32), _ptr(mix, torch.float32), _ptr(out, torch.float32), _ptr(h, torch.float32), B, n, D, act,
                                  _ptr(h_out), _stream()), "gymrl_mhc_combine")
    return h_out


def rmsnorm(x, w, eps, n_sum=1, act=0):
    """gymrl_rmsnorm: x [B, n_sum * D] (or [B, n_sum, D]) -> y [B, D] = s rsqrt(mean(s^2) + eps) w, s = act(the sum of the blocks)."""
    B, D = x.shape[0], w.numel()
    y = torch.empty(B, D, device=x.device)
    check(lib().gymrl_rmsnorm(_ptr(x, torch.float32), _ptr(w, torch.float32), B, D, n_sum, eps, act, _ptr(y), _stream()), "gymrl_rmsnorm")
    return y


_SCRATCH_MAX = 64
_scratch_cache = collections.OrderedDict()


def _scratch(kind, shape_key, nbytes, dev):
    """Partial-sum scratch of the backward kernels that take one.  Cached per (kernel, shape, device, STREAM): two
    streams never share a buffer, so concurrent backward passes cannot race on it.  While the stream is capturing a
    hipGraph a missing buffer is allocated for this call only (it then lives in the graph's private pool like any other
    temporary) and is NOT cached — an eager call after `del graph` must never inherit memory of a dead graph's pool.
    The cache is a bounded LRU (_SCRATCH_MAX entries): code that keeps creating streams cannot grow it without limit, and
    an evicted buffer goes back to torch's caching allocator, which hands a block to another stream only after the work
    queued on the allocating stream (the one in the key) has been ordered before the reuse — so a raw stream handle that
    is recycled after its stream died finds either its own old buffer (same stream-ordering domain) or none."""
    key = (kind, shape_key, dev, torch.cuda.current_stream(dev).cuda_stream)
    ws = _scratch_cache.get(key)
    if ws is not None:
        _scratch_cache.move_to_end(key)
        return ws
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    if not torch.cuda.is_current_stream_capturing():
        _scratch_cache[key] = ws
        while len(_scratch_cache) > _SCRATCH_MAX:
            _scratch_cache.popitem(last=False)
    return ws


def rmsnorm_bwd(g, x, w, eps, act=0, n_sum=1):
    """gymrl_rmsnorm_bwd / gymrl_rmsnorm_sum_bwd: (dL/dx [B, D], dL/dw [D]) of y = rmsnorm(x, w, eps, act=act); D <= 512.
    n_sum > 1: x is [B, n_sum, D] and the norm is of the blocks' sum — dL/dx [B, D] is every block's gradient."""
    B, D = x.shape[0], w.numel()
    ws = _scratch("rmsnorm_bwd", D, lib().gymrl_rmsnorm_bwd_workspace_bytes(D), x.device)
    d_x, d_w = torch.empty(B, D, device=x.device), torch.empty_like(w)
    check(lib().gymrl_rmsnorm_sum_bwd(_ptr(g, torch.float32), _ptr(x, torch.float32), _ptr(w, torch.float32), B, D, n_sum, eps, act, _ptr(d_x),
                                      _ptr(d_w), _ptr(ws), _stream()), "gymrl_rmsnorm_sum_bwd")
    return d_x, d_w


def norm_proj_ok(D, n_out):
    """Shapes gymrl_norm_proj_fwd / _bwd take."""
    return 0 < D <= 256 and 0 < n_out <= 8


def _al16(t):
    """A tensor whose storage starts on a 16-byte boundary (a copy if the view does not): the D = 256 head-tail kernels are
    chosen by shape alone and require it (-22 otherwise), so that a result's bits never depend on where a view starts."""
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def norm_proj_fwd(x, norm_w, eps, W2, b2):
    """gymrl_norm_proj_fwd: RMSNorm(SiLU(x)) W2^T + b2 -> [B, n_out] in one launch."""
    B, D = x.shape
    if D == 256:
        x, norm_w, W2 = _al16(x), _al16(norm_w), _al16(W2)
    out = torch.empty(B, W2.shape[0], device=x.device)
    f = torch.float32
    check(lib().gymrl_norm_proj_fwd(_ptr(x, f), _ptr(norm_w, f), _ptr(W2, f), _ptr(b2, f, True), B, D, W2.shape[0], eps, _ptr(out), _stream()),
          "gymrl_norm_proj_fwd")
    return out


def norm_proj_bwd(d_out, x, norm_w, eps, W2):
    """gymrl_norm_proj_bwd -> (d_x, d_norm_w, d_W2, d_b2)."""
    B, D = x.shape
    n_out = W2.shape[0]
    if D == 256:
        x, norm_w, W2 = _al16(x), _al16(norm_w), _al16(W2)
    ws = _scratch("norm_proj_bwd", (D, n_out), lib().gymrl_norm_proj_bwd_workspace_bytes(D, n_out), x.device)
    d_x, d_nw, d_W2 = torch.empty_like(x), torch.empty_like(norm_w), torch.empty_like(W2)
    d_b2 = torch.empty(n_out, device=x.device)
    f = torch.float32
    check(lib().gymrl_norm_proj_bwd(_ptr(d_out, f), _ptr(x, f), _ptr(norm_w, f), _ptr(W2, f), B, D, n_out, eps, _ptr(d_x), _ptr(d_nw), _ptr(d_W2),
                                    _ptr(d_b2), _ptr(ws), _stream()), "gymrl_norm_proj_bwd")
    return d_x, d_nw, d_W2, d_b2


def mhc_sub_forward(h, norm_w, w, alpha, beta, lin_w, lin_b, sk_it):
    """gymrl_mhc_sub_forward: one hyper-connection sub-block forward (n = 2, D = 128) in one launch ->
    (pre, post, mix, stats, read, z, h_out).  h [B, 2, D], or [B, D]: the same row for both branches."""
    B, n, D = (h.shape[0], 2, h.shape[1]) if h.dim() == 2 else h.shape
    dev = h.device
    pre, post, mix = torch.empty(B, n, device=dev), torch.empty(B, n, device=dev), torch.empty(B, n, n, device=dev)
    stats, read, z = torch.empty(B, n * n + 2 * n + 1, device=dev), torch.empty(B, D, device=dev), torch.empty(B, D, device=dev)
    h_out = torch.empty(B, n, D, device=dev)
    f = torch.float32
    check(lib().gymrl_mhc_sub_forward(_ptr(h, f), h.dim() == 2, _ptr(norm_w, f), _ptr(w, f), _ptr(alpha, f), _ptr(beta, f), _ptr(lin_w, f),
                                      _ptr(lin_b, f), B, n, D, sk_it, _ptr(pre), _ptr(post), _ptr(mix), _ptr(stats), _ptr(read), _ptr(z), _ptr(h_out),
                                      _stream()), "gymrl_mhc_sub_forward")
    return pre, post, mix, stats, read, z, h_out


def mhc_sub_backward(g, h, z, pre, post, mix, stats, norm_w, w, alpha, lin_w, sum_branches=False):
    """gymrl_mhc_sub_backward: one hyper-connection sub-block backward (n = 2, D = 128) in one launch ->
    (d_z, d_h, d_norm_w, d_w, d_alpha, d_beta).  g / h may be [B, 128] (the same row for both branches); sum_branches: d_h
    comes back [B, 128], the branches' gradients added."""
    B, D = z.shape
    dev = z.device
    f = torch.float32
    for t, nm in ((g, "g"), (h, "h")):
        if t.shape not in ((B, 2, D), (B, D)) or not t.is_contiguous():
            raise ValueError(f"{nm}: expected a contiguous [B, 2, D] or [B, D] tensor")
    ws = _scratch("mhc_gates_bwd", (2, D), lib().gymrl_mhc_gates_bwd_workspace_bytes(2, D), dev)
    Bp = (B + 15) // 16 * 16                               # the kernel writes whole 16-row tiles
    d_z = torch.empty(Bp, D, device=dev)[:B]
    d_h = (torch.empty(Bp, D, device=dev) if sum_branches else torch.empty(Bp, 2, D, device=dev))[:B]
    d_nw, d_w = torch.empty_like(norm_w), torch.empty_like(w)
    d_alpha, d_beta = torch.empty(3, device=dev), torch.empty(w.shape[1], device=dev)
    check(lib().gymrl_mhc_sub_backward(_ptr(g, f), g.dim() == 2, _ptr(h, f), h.dim() == 2, _ptr(z, f), _ptr(pre, f), _ptr(post, f), _ptr(mix, f),
                                       _ptr(stats, f), _ptr(norm_w, f), _ptr(w, f), _ptr(alpha, f), _ptr(lin_w, f), B, 2, D, _ptr(d_z), _ptr(d_h),
                                       bool(sum_branches), _ptr(d_nw), _ptr(d_w), _ptr(d_alpha), _ptr(d_beta), _ptr(ws), _stream()),
          "gymrl_mhc_sub_backward")
    return d_z, d_h, d_nw, d_w, d_alpha, d_beta


def mhc_policy(desc, obs, logits_out=None, value_out=None):
    """gymrl_mhc_policy_forward: PPO-full's whole rollout forward in one launch.  desc: a filled _lib.MhcPolicy (its pointers
    must stay alive: they are the modules' parameters); obs [B, obs_dim] -> (logits [B, n_act], value [B])."""
    B = obs.shape[0]
    logits = torch.empty(B, desc.n_act, device=obs.device) if logits_out is None else logits_out
    value = torch.empty(B, device=obs.device) if value_out is None else value_out
    check(lib().gymrl_mhc_policy_forward(C.byref(desc), _ptr(obs, torch.float32), B, _ptr(logits, torch.float32), _ptr(value, torch.float32),
                                         _stream()), "gymrl_mhc_policy_forward")
    return logits, value


def mhc_policy_pack(desc, image=None):
    """gymrl_mhc_policy_pack: the image of desc's wide operands (the sub-blocks' Linears and gate weights, the heads' first
    Linears) in the order the one-launch forward's lanes read them; returns the buffer (desc.image is the caller's to set —
    and to refresh: the image does not follow the parameters)."""
    n = int(lib().gymrl_mhc_policy_image_floats(desc.n_sub))
    if image is None or image.numel() != n:
        image = torch.empty(n, dtype=torch.float32, device=torch.device("cuda", torch.cuda.current_device()))
    check(lib().gymrl_mhc_policy_pack(C.byref(desc), _ptr(image, torch.float32), _stream()), "gymrl_mhc_policy_pack")
    return image


def sinkhorn(A, sk_it):
    """gymrl_sinkhorn: A [B, n, n] -> (u [B, n], v [B, n])."""
    B, n, _ = A.shape
    u, v = torch.empty(B, n, device=A.device), torch.empty(B, n, device=A.device)
    check(lib().gymrl_sinkhorn(_ptr(A, torch.float32), B, n, sk_it, _ptr(u), _ptr(v), _stream()), "gymrl_sinkhorn")
    return u, v


def mhc_read_fwd(pre, h):
    B, n, D = h.shape
    read = torch.empty(B, D, device=h.device)
    check(lib().gymrl_mhc_read_fwd(_ptr(pre, torch.float32), _ptr(h, torch.float32), B, n, D, _ptr(read), _stream()), "gymrl_mhc_read_fwd")
    return read


def mhc_read_bwd(g, pre, h, want_dh=True):
    """(d_pre, d_h); want_dh=False: d_pre only (the d_h term goes through gymrl_mhc_gates_bwd's d_read)."""
    B, n, D = h.shape
    d_pre = torch.empty(B, n, device=h.device)
    d_h = torch.empty_like(h) if want_dh else None
    check(lib().gymrl_mhc_read_bwd(_ptr(g, torch.float32), _ptr(pre, torch.float32), _ptr(h, torch.float32), B, n, D, _ptr(d_pre),
                                   None if d_h is None else _ptr(d_h), 0, _stream()), "gymrl_mhc_read_bwd")
    return d_pre, d_h


def mhc_combine_bwd(g, post, mix, out, h, act=0, want_dh=True):
    """(d_post, d_mix, d_out, d_h) of gymrl_mhc_combine with the same act (silu: `out` is the raw z and d_out is dL/dz);
    want_dh=False: d_h = None (left to gymrl_mhc_gates_bwd's g_out term)."""
    B, n, D = h.shape
    dev = h.device
    d_post, d_mix = torch.empty(B, n, device=dev), torch.empty(B, n, n, device=dev)
    d_out = torch.empty(B, D, device=dev)
    d_h = torch.empty_like(h) if want_dh else None
    check(lib().gymrl_mhc_combine_bwd(_ptr(g, torch.float32), _ptr(post, torch.float32), _ptr(mix, torch.float32), _ptr(out, torch.float32),
                                      _ptr(h, torch.float32), B, n, D, act, _ptr(d_post), _ptr(d_mix), _ptr(d_out),
                                      None if d_h is None else _ptr(d_h), _stream()), "gymrl_mhc_combine_bwd")
    return d_post, d_mix, d_out, d_h


def mhc_gates_bwd(h, norm_w, w, alpha, pre, post, mix, stats, d_pre, d_post, d_mix, d_read=None, g_out=None):
    """gymrl_mhc_gates_bwd -> (d_h, d_norm_w, d_w, d_alpha, d_beta); n = 2 branches, n * D in (256, 512).  d_read [B, D] /
    g_out [B, n, D]: the read's and the combine's gradient paths into h, folded into d_h in the same pass."""
    B, n, D = h.shape
    dev = h.device
    ws = _scratch("mhc_gates_bwd", (n, D), lib().gymrl_mhc_gates_bwd_workspace_bytes(n, D), dev)
    d_h, d_nw, d_w = torch.empty_like(h), torch.empty_like(norm_w), torch.empty_like(w)
    d_alpha, d_beta = torch.empty(3, device=dev), torch.empty(w.shape[1], device=dev)
    opt = lambda t: None if t is None else _ptr(t, torch.float32)   # noqa: E731
    check(lib().gymrl_mhc_gates_bwd(_ptr(h, torch.float32), _ptr(norm_w, torch.float32), _ptr(w, torch.float32), _ptr(alpha, torch.float32),
                                    _ptr(pre, torch.float32), _ptr(post, torch.float32), _ptr(mix, torch.float32), _ptr(stats, torch.float32),
                                    _ptr(d_pre, torch.float32), _ptr(d_post, torch.float32), _ptr(d_mix, torch.float32), opt(d_read), opt(g_out), B,
                                    n, D, _ptr(d_h), _ptr(d_nw), _ptr(d_w), _ptr(d_alpha), _ptr(d_beta), _ptr(ws), _stream()), "gymrl_mhc_gates_bwd")
    return d_h, d_nw, d_w, d_alpha, d_beta


# ------------------------------------------------- fused SAC vector step ---
def _addr(t):
    return None if t is None else _ptr(t).value


FUSED_MAX_BATCH = 8192     # row-slab kernels: B <= 256 as resident 2-D grids, above that slab-adjacent 1-D grids (slab_step_device.hpp slab_grid)


# What the five row-slab steps' bindings below share (slab_step_device.hpp slab_shape_ok is the library's side of the first)
def _fused_shape_ok(B, D, A, H, max_batch, max_A):
    return 0 < B <= max_batch and 0 < D <= 8 and 0 < A <= max_A and 4 <= H <= 256 and H % 4 == 0


def _zeroed_workspace(nbytes, device):
    return torch.zeros(int(nbytes), dtype=torch.uint8, device=device)


def _set_ring(a, ring):
    a.r_state, a.r_action, a.r_reward, a.r_next, a.r_flag = (_addr(t) for t in ring)


def _set_optimisers(a, betas_from, **opts):
    """a.<name>_p / _m / _v: each FusedAdam's flat parameter buffer and its moments; betas and eps as `betas_from` has them."""
    for name, opt in opts.items():
        for f in "pmv":
            setattr(a, f"{name}_{f}", _addr(getattr(opt, f)))
    g = betas_from.param_groups[0]
    a.beta1, a.beta2, a.eps_adam = g["betas"][0], g["betas"][1], g["eps"]


def _set_adam_bias(a, **blocks):
    """adam_bias() blocks (16 bytes each) into a's float[4] fields of those names; None leaves a field as it is."""
    for name, blk in blocks.items():
        if blk is not None:
            getattr(a, name)[:] = (C.c_float * 4).from_buffer_copy(blk)[:]


def _set_draw(a, idx, idx_seed, idx_counter, idx_size, idx_dev):
    a.idx, a.idx_seed, a.idx_counter, a.idx_size, a.idx_dev = _addr(idx), idx_seed, idx_counter, idx_size, _addr(idx_dev)


def _set_act_env(a, env, actor, ring, cap, images):
    """An act step's fixed fields: the env, the shapes, the replay ring and the actor's fc2 image."""
    a.N, a.D, a.A, a.H = env.n, env.obs_dim, env.act_dim, actor.fc1.weight.shape[0]
    a.env_kind, a.env_state, a.env_seed, a.env_id0 = env.kind, _addr(env.state), env.seed, env.env_id0
    _set_ring(a, ring)
    a.cap, a.images = cap, _addr(images)


def _classic_act_entry(name, kind):
    """The entry point of an act launch on env kind `kind`: CartPole-v1 keeps the one it has always called, MountainCar-v0 and
    Acrobot-v1 (FUSED_ACT_KINDS) take its `_classic` sibling; any other kind goes to `name`, which refuses it."""
    return name + "_classic" if kind in FUSED_ACT_KINDS and kind != CARTPOLE else name


def _set_act_io(a, env, obs, obs_out, cursor, cursor_dev, outs):
    """An act step's per-call fields; outs = (action_out, rew_out, done_out, ep_ret_out, ep_stats), each a tensor or None."""
    a.env_seed = env.seed                              # reset(seed=...) may have moved it
    a.obs, a.obs_out = _ptr(obs, torch.float32).value, _ptr(obs_out, torch.float32).value
    a.cursor, a.cursor_dev = cursor, _addr(cursor_dev)
    a.action_out, a.rew_out, a.done_out, a.ep_ret_out, a.ep_stats = (_addr(t) for t in outs)


def sac_fused_shape_ok(B, D, A, H):
    """Shapes gymrl_sac_act_step / gymrl_sac_update take (include/gymrl.h): everything else runs layer by layer."""
    return _fused_shape_ok(B, D, A, H, FUSED_MAX_BATCH, 4)


def sac_update_workspace(B, D, A, H, device):
    # zeroed: the hand-off flags between the row phases' workgroups and the large-batch grids' tickets live in it (zero before
    # the first launch, left zero)
    return _zeroed_workspace(lib().gymrl_sac_update_workspace_bytes(B, D, A, H), device)


def _sac_actor_params(dst, actor):
    for k, layer in enumerate((actor.fc1, actor.fc2, actor.mean, actor.log_std)):
        dst.w[k], dst.b[k] = _addr(layer.weight), _addr(layer.bias)


def _sac_critic_params(dst, critic):
    for k, layer in enumerate((critic.fc1, critic.fc2, critic.fc3, critic.fc4, critic.fc5, critic.fc6)):
        dst.w[k], dst.b[k] = _addr(layer.weight), _addr(layer.bias)


def sac_act_args(env, actor, ring, cap, bound, log_std_min, log_std_max, images=None):
    """A gymrl_sac_act_args with everything that does not change from step to step filled in (env, actor parameters —
    views of a flat buffer the optimiser updates in place — and the replay ring)."""
    a = SacActArgs()
    _set_act_env(a, env, actor, ring, cap, images)
    a.bound, a.log_std_min, a.log_std_max = float(bound), float(log_std_min), float(log_std_max)
    _sac_actor_params(a.actor, actor)
    return a


def sac_act_step(a, env, obs, obs_out, cursor=0, cursor_dev=None, eps=None, noise_seed=0, noise_counter=0, noise_counter_dev=None,
                 action_out=None, rew_out=None, done_out=None, ep_ret_out=None, ep_stats=None):
    """gymrl_sac_act_step: Actor forward on obs [N, D], reparameterised draw, env step with auto-reset, replay rows at
    (cursor + env) % cap — ONE launch (sac_pendulum.py:278-283)."""
    _set_act_io(a, env, obs, obs_out, cursor, cursor_dev, (action_out, rew_out, done_out, ep_ret_out, ep_stats))
    a.eps = _addr(eps)
    a.noise_seed, a.noise_counter, a.noise_counter_dev = noise_seed, noise_counter, _addr(noise_counter_dev)
    check(lib().gymrl_sac_act_step(C.byref(a), _stream()), "gymrl_sac_act_step")


def sac_images(H, device):
    """The eight weight images of the H x H layers (gymrl_sac_update_args.images), or None when H % 16 != 0."""
    return torch.zeros(8 * H * H, device=device) if H % 16 == 0 else None


def sac_pack_images(a):
    """gymrl_sac_pack_images: rebuild every image from the parameters as they are now."""
    check(lib().gymrl_sac_pack_images(C.byref(a), _stream()), "gymrl_sac_pack_images")


def sac_update_args(B, D, A, actor, critic, target, actor_opt, critic_opt, ring, cfg_scalars, log_alpha, alpha_m, alpha_v, sums,
                    alpha_loss, workspace, images=None):
    """A gymrl_sac_update_args with the per-trainer constants filled in.  cfg_scalars = (gamma, tau, bound, log_std_min,
    log_std_max, target_entropy, lr_alpha); actor_opt / critic_opt: FusedAdam over the modules' flat buffers."""
    a = SacUpdateArgs()
    a.B, a.D, a.A, a.H = B, D, A, actor.fc1.weight.shape[0]
    gamma, tau, bound, lo, hi, tent, lr_alpha = cfg_scalars
    a.gamma, a.tau, a.bound, a.log_std_min, a.log_std_max, a.target_entropy = float(gamma), float(tau), float(bound), float(lo), float(hi), float(tent)
    _set_ring(a, ring)
    _sac_actor_params(a.actor, actor)
    _sac_critic_params(a.critic, critic)
    _sac_critic_params(a.target, target)
    _set_optimisers(a, critic_opt, actor=actor_opt, critic=critic_opt)
    a.log_alpha, a.alpha_m, a.alpha_v, a.lr_alpha = _addr(log_alpha), _addr(alpha_m), _addr(alpha_v), float(lr_alpha)
    a.sums, a.alpha_loss, a.workspace = _addr(sums), _addr(alpha_loss), _addr(workspace)
    a.images = _addr(images)
    return a


def sac_update(a, idx=None, idx_seed=0, idx_counter=0, idx_size=0, idx_dev=None, eps_next=None, eps_cur=None, noise_seed=0,
               noise_counter=0, noise_counter_dev=None, adam_critic=None, adam_actor=None, adam_critic_dev=None, adam_actor_dev=None,
               alpha_bias=(1.0, 1.0), alpha_bias_dev=None):
    """gymrl_sac_update: SACTrainer.update() (sac_pendulum.py:213-267) as four launches.  adam_critic / adam_actor: the
    16-byte blocks of adam_bias() (host) or device views of them; alpha_bias = (1 - 0.9^t, 1 - 0.999^t)."""
    _set_draw(a, idx, idx_seed, idx_counter, idx_size, idx_dev)
    a.eps_next, a.eps_cur = _addr(eps_next), _addr(eps_cur)
    a.noise_seed, a.noise_counter, a.noise_counter_dev = noise_seed, noise_counter, _addr(noise_counter_dev)
    _set_adam_bias(a, adam_critic=adam_critic, adam_actor=adam_actor)
    a.adam_critic_dev, a.adam_actor_dev = _addr(adam_critic_dev), _addr(adam_actor_dev)
    a.alpha_bias[0], a.alpha_bias[1], a.alpha_bias_dev = alpha_bias[0], alpha_bias[1], _addr(alpha_bias_dev)
    check(lib().gymrl_sac_update(C.byref(a), _stream()), "gymrl_sac_update")


# ------------------------------------------ fused TD3 / DDPG vector step ---
TD3_FUSED_MAX_BATCH = 256      # one grid of at most 16 slabs per row phase (td3_step.hip kTd3MaxBatch)


def td3_fused_shape_ok(B, D, A, H):
    """Shapes gymrl_td3_act_step / gymrl_td3_update take (include/gymrl.h): everything else runs layer by layer."""
    return _fused_shape_ok(B, D, A, H, TD3_FUSED_MAX_BATCH, 4)


def td3_update_workspace(B, D, A, H, device):
    return _zeroed_workspace(lib().gymrl_td3_update_workspace_bytes(B, D, A, H), device)


def _td3_actor_params(dst, actor):
    for k, layer in enumerate((actor.fc1, actor.fc2, actor.fc3)):
        dst.w[k], dst.b[k] = _addr(layer.weight), _addr(layer.bias)


def _td3_critic_params(dst, critic):
    """TD3's twin module fills fc1..fc6, DDPG's single Q network fc1..fc3 (the rest stays NULL)."""
    for k, name in enumerate(("fc1", "fc2", "fc3", "fc4", "fc5", "fc6")):
        layer = getattr(critic, name, None)
        if layer is not None:
            dst.w[k], dst.b[k] = _addr(layer.weight), _addr(layer.bias)


def td3_images(H, device):
    """The nine weight images of the H x H layers (gymrl_td3_update_args.images), or None when H % 16 != 0."""
    return torch.zeros(9 * H * H, device=device) if H % 16 == 0 else None


def td3_pack_images(a):
    """gymrl_td3_pack_images: rebuild every image from the parameters as they are now."""
    check(lib().gymrl_td3_pack_images(C.byref(a), _stream()), "gymrl_td3_pack_images")


def td3_act_args(env, actor, ring, cap, bound, noise_std, images=None):
    """A gymrl_td3_act_args with everything that does not change from step to step filled in.  noise_std: the exploration
    std select_action() passes to noisy_action (exploration noise times the action bound)."""
    if tuple(ring[0].shape[1:]) != (env.obs_dim,) or tuple(ring[1].shape[1:]) != (env.act_dim,):
        raise ValueError(f"td3_act_args: ring rows {tuple(ring[0].shape)} / {tuple(ring[1].shape)} do not fit the env")
    a = Td3ActArgs()
    _set_act_env(a, env, actor, ring, cap, images)
    a.bound, a.noise_std = float(bound), float(noise_std)
    _td3_actor_params(a.actor, actor)
    return a


def td3_act_step(a, env, obs, obs_out, cursor=0, cursor_dev=None, eps=None, noise_seed=0, noise_counter=0, noise_counter_dev=None,
                 action_out=None, rew_out=None, done_out=None, ep_ret_out=None, ep_stats=None):
    """gymrl_td3_act_step: actor forward on obs [N, D], exploration noise (noisy_action mode 0; eps = f64[N, A] or None:
    Philox (noise_seed, noise_counter)), env step with auto-reset, replay rows at (cursor + env) % cap — ONE launch."""
    if tuple(obs.shape) != (a.N, a.D) or tuple(obs_out.shape) != (a.N, a.D):
        raise ValueError(f"td3_act_step: obs {tuple(obs.shape)} / obs_out {tuple(obs_out.shape)}, expected {(a.N, a.D)}")
    if eps is not None and (eps.dtype != torch.float64 or eps.numel() != a.N * a.A):
        raise ValueError("td3_act_step: eps must be float64 [N, A]")
    _set_act_io(a, env, obs, obs_out, cursor, cursor_dev, (action_out, rew_out, done_out, ep_ret_out, ep_stats))
    a.eps = None if eps is None else _ptr(eps, torch.float64).value
    a.noise_seed, a.noise_counter, a.noise_counter_dev = noise_seed, noise_counter, _addr(noise_counter_dev)
    check(lib().gymrl_td3_act_step(C.byref(a), _stream()), "gymrl_td3_act_step")


def td3_update_args(B, D, A, n_critics, actor, actor_target, critic, critic_target, actor_opt, critic_opt, ring, cfg_scalars, sums,
                    workspace, images=None):
    """A gymrl_td3_update_args with the per-trainer constants filled in.  cfg_scalars = (gamma, tau, bound, policy_noise,
    noise_clip); sums: f64[2] (critic loss sum, sum of Q(s, actor(s)))."""
    if sums.dtype != torch.float64 or sums.numel() != 2 or not sums.is_contiguous():
        raise ValueError("td3_update_args: sums must be a contiguous float64[2]")
    if tuple(ring[0].shape[1:]) != (D,) or tuple(ring[1].shape[1:]) != (A,):
        raise ValueError(f"td3_update_args: ring rows {tuple(ring[0].shape)} / {tuple(ring[1].shape)}, expected [.., {D}] / [.., {A}]")
    a = Td3UpdateArgs()
    a.B, a.D, a.A, a.H, a.n_critics = B, D, A, actor.fc1.weight.shape[0], n_critics
    gamma, tau, bound, policy_noise, noise_clip = cfg_scalars
    a.gamma, a.tau, a.bound, a.policy_noise, a.noise_clip = float(gamma), float(tau), float(bound), float(policy_noise), float(noise_clip)
    _set_ring(a, ring)
    _td3_actor_params(a.actor, actor)
    _td3_actor_params(a.actor_target, actor_target)
    _td3_critic_params(a.critic, critic)
    _td3_critic_params(a.critic_target, critic_target)
    _set_optimisers(a, critic_opt, actor=actor_opt, critic=critic_opt)
    a.sums, a.workspace, a.images = _addr(sums), _addr(workspace), _addr(images)
    return a


def td3_update(a, idx=None, idx_seed=0, idx_counter=0, idx_size=0, idx_dev=None, eps=None, noise_seed=0, noise_counter=0,
               noise_counter_dev=None, delayed=1, delayed_dev=None, adam_critic=None, adam_actor=None, adam_critic_dev=None,
               adam_actor_dev=None):
    """gymrl_td3_update: TD3Trainer.update() / DDPGTrainer.update() as at most four launches.  idx: i32[B] rows or None (the
    keyed draw); eps: f64[B, A] smoothing draws or None (Philox); delayed / delayed_dev (i32[1]): whether the actor phases run;
    adam_critic / adam_actor: the 16-byte blocks of adam_bias() (host) or device views of them."""
    if idx is not None and (idx.dtype != torch.int32 or idx.numel() != a.B):
        raise ValueError(f"td3_update: idx must be int32 [{a.B}]")
    if eps is not None and (eps.dtype != torch.float64 or eps.numel() != a.B * a.A):
        raise ValueError(f"td3_update: eps must be float64 [{a.B}, {a.A}]")
    _set_draw(a, idx, idx_seed, idx_counter, idx_size, idx_dev)
    a.eps = _addr(eps)
    a.noise_seed, a.noise_counter, a.noise_counter_dev = noise_seed, noise_counter, _addr(noise_counter_dev)
    a.delayed, a.delayed_dev = int(bool(delayed)), _addr(delayed_dev)
    _set_adam_bias(a, adam_critic=adam_critic, adam_actor=adam_actor)
    a.adam_critic_dev, a.adam_actor_dev = _addr(adam_critic_dev), _addr(adam_actor_dev)
    check(lib().gymrl_td3_update(C.byref(a), _stream()), "gymrl_td3_update")


# --------------------------------------- fused discrete-SAC vector step ---
DSAC_FUSED_MAX_BATCH = 256     # one grid of at most 16 slabs per row phase (dsac_step.hip kDsacMaxBatch)


def dsac_fused_shape_ok(B, D, A, H):
    """Shapes gymrl_dsac_act_step / gymrl_dsac_update take (include/gymrl.h): everything else runs layer by layer."""
    return _fused_shape_ok(B, D, A, H, DSAC_FUSED_MAX_BATCH, 4)


class _SoftmaxRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z):
        z = z.contiguous()
        B, A = z.shape
        p = torch.empty_like(z)
        check(lib().gymrl_softmax_rows_fwd(_ptr(z, torch.float32), B, A, _ptr(p), _stream()), "gymrl_softmax_rows_fwd")
        ctx.save_for_backward(p)
        return p

    @staticmethod
    def backward(ctx, g):
        p, = ctx.saved_tensors
        g = g.contiguous()
        B, A = p.shape
        dz = torch.empty_like(p)
        check(lib().gymrl_softmax_rows_bwd(_ptr(p, torch.float32), _ptr(g, torch.float32), B, A, _ptr(dz), _stream()), "gymrl_softmax_rows_bwd")
        return dz


def softmax_rows(z):
    """softmax over the last dimension of z f32[B, A] (A <= 8) with csrc/softmax_device.hpp's arithmetic, forward and
    backward: the bits the fused discrete-SAC step produces (F.softmax's belong to torch)."""
    if z.dim() != 2 or not 0 < z.shape[1] <= 8:
        raise ValueError(f"softmax_rows: expected [B, A <= 8], got {tuple(z.shape)}")
    return _SoftmaxRows.apply(z)


def dsac_update_workspace(B, D, A, H, device):
    return _zeroed_workspace(lib().gymrl_dsac_update_workspace_bytes(B, D, A, H), device)


def dsac_images(H, device):
    """The eight weight images of the H x H layers (gymrl_dsac_update_args.images), or None when H % 16 != 0."""
    return torch.zeros(8 * H * H, device=device) if H % 16 == 0 else None


def dsac_pack_images(a):
    """gymrl_dsac_pack_images: rebuild every image from the parameters as they are now."""
    check(lib().gymrl_dsac_pack_images(C.byref(a), _stream()), "gymrl_dsac_pack_images")


def dsac_act_args(env, actor, ring, cap, images=None):
    """A gymrl_dsac_act_args with everything that does not change from step to step filled in."""
    if tuple(ring[0].shape[1:]) != (env.obs_dim,) or tuple(ring[1].shape[1:]) != (1,):
        raise ValueError(f"dsac_act_args: ring rows {tuple(ring[0].shape)} / {tuple(ring[1].shape)} do not fit the env")
    a = DsacActArgs()
    _set_act_env(a, env, actor, ring, cap, images)
    _td3_actor_params(a.actor, actor)
    return a


def dsac_act_step(a, env, obs, obs_out, cursor=0, cursor_dev=None, noise_exp=None, seed=0, counter=0, counter_dev=None,
                  action_out=None, rew_out=None, done_out=None, ep_ret_out=None, ep_stats=None, entry=None):
    """gymrl_dsac_act_step: actor logits on obs [N, D], the categorical draw (noise_exp = f32[N, A] Exp(1) draws or None:
    gymrl_categorical_sample's Philox keys under (seed, counter)), the env's step with auto-reset (CartPole-v1; MountainCar-v0
    and Acrobot-v1 through gymrl_dsac_act_step_classic, or whichever of the two `entry` names), replay rows at
    (cursor + env) % cap — ONE launch."""
    if tuple(obs.shape) != (a.N, a.D) or tuple(obs_out.shape) != (a.N, a.D):
        raise ValueError(f"dsac_act_step: obs {tuple(obs.shape)} / obs_out {tuple(obs_out.shape)}, expected {(a.N, a.D)}")
    if noise_exp is not None and (noise_exp.dtype != torch.float32 or noise_exp.numel() != a.N * a.A):
        raise ValueError("dsac_act_step: noise_exp must be float32 [N, A]")
    if action_out is not None and (action_out.dtype != torch.int32 or action_out.numel() != a.N):
        raise ValueError("dsac_act_step: action_out must be int32 [N]")
    _set_act_io(a, env, obs, obs_out, cursor, cursor_dev, (action_out, rew_out, done_out, ep_ret_out, ep_stats))
    a.noise_exp = _addr(noise_exp)
    a.seed, a.counter, a.counter_dev = seed, counter, _addr(counter_dev)
    entry = entry or _classic_act_entry("gymrl_dsac_act_step", a.env_kind)
    check(getattr(lib(), entry)(C.byref(a), _stream()), entry)


def dsac_update_args(B, D, A, actor, critic1, critic2, critic1_target, critic2_target, actor_opt, critic1_opt, critic2_opt, ring,
                     cfg_scalars, log_alpha, alpha_m, alpha_v, sums, alpha_loss, workspace, images=None):
    """A gymrl_dsac_update_args with the per-trainer constants filled in.  cfg_scalars = (gamma, tau, target_entropy,
    lr_alpha); sums: f64[4] (critic1, critic2 loss sums, actor loss sum, entropy sum)."""
    if sums.dtype != torch.float64 or sums.numel() != 4 or not sums.is_contiguous():
        raise ValueError("dsac_update_args: sums must be a contiguous float64[4]")
    if tuple(ring[0].shape[1:]) != (D,) or tuple(ring[1].shape[1:]) != (1,):
        raise ValueError(f"dsac_update_args: ring rows {tuple(ring[0].shape)} / {tuple(ring[1].shape)}, expected [.., {D}] / [.., 1]")
    a = DsacUpdateArgs()
    a.B, a.D, a.A, a.H = B, D, A, actor.fc1.weight.shape[0]
    gamma, tau, tent, lr_alpha = cfg_scalars
    a.gamma, a.tau, a.target_entropy = float(gamma), float(tau), float(tent)
    _set_ring(a, ring)
    for dst, net in ((a.actor, actor), (a.critic1, critic1), (a.critic2, critic2), (a.critic1_target, critic1_target),
                     (a.critic2_target, critic2_target)):
        _td3_actor_params(dst, net)
    _set_optimisers(a, critic1_opt, actor=actor_opt, critic1=critic1_opt, critic2=critic2_opt)
    a.log_alpha, a.alpha_m, a.alpha_v = (_ptr(t, torch.float32).value for t in (log_alpha, alpha_m, alpha_v))
    a.lr_alpha, a.alpha_beta1, a.alpha_beta2, a.alpha_eps = float(lr_alpha), 0.9, 0.999, 1e-8      # dsac_alpha_step's defaults
    a.sums, a.alpha_loss, a.workspace, a.images = _addr(sums), _addr(alpha_loss), _addr(workspace), _addr(images)
    return a


def dsac_update(a, idx=None, idx_seed=0, idx_counter=0, idx_size=0, idx_dev=None, adam_critic1=None, adam_critic2=None, adam_actor=None,
                adam_critic1_dev=None, adam_critic2_dev=None, adam_actor_dev=None, alpha_t=0, alpha_bias_dev=None):
    """gymrl_dsac_update: sac_cartpole.SACTrainer.update() as four launches.  idx: i32[B] rows or None (the keyed draw);
    adam_*: the 16-byte blocks of adam_bias() (host) or device views of them; alpha_t: the temperature's step count, or
    alpha_bias_dev = f64[2] {1 - b1^t, 1 - b2^t} on the device."""
    if idx is not None and (idx.dtype != torch.int32 or idx.numel() != a.B):
        raise ValueError(f"dsac_update: idx must be int32 [{a.B}]")
    _set_draw(a, idx, idx_seed, idx_counter, idx_size, idx_dev)
    _set_adam_bias(a, adam_critic1=adam_critic1, adam_critic2=adam_critic2, adam_actor=adam_actor)
    a.adam_critic1_dev, a.adam_critic2_dev, a.adam_actor_dev = _addr(adam_critic1_dev), _addr(adam_critic2_dev), _addr(adam_actor_dev)
    a.alpha_t, a.alpha_bias_dev = int(alpha_t), _addr(alpha_bias_dev)
    check(lib().gymrl_dsac_update(C.byref(a), _stream()), "gymrl_dsac_update")


# ------------------------------------------------- fused DQN vector step ---
DQN_FUSED_MAX_BATCH = 256      # one grid of at most 16 slabs in the row phase (dqn_step.hip kDqnMaxBatch)


def dqn_fused_shape_ok(B, D, A, H):
    """Shapes gymrl_dqn_act_step / gymrl_dqn_update take (include/gymrl.h): everything else runs layer by layer."""
    return _fused_shape_ok(B, D, A, H, DQN_FUSED_MAX_BATCH, 4)


class _Layers3:
    """Three Linear layers under the names the shared helpers read: dqn_cartpole.QNetwork's (net.0, net.2, net.4), or a tuple
    (fc1, fc2, fc3) — the dueling net's (fc1, value_stream, advantage_stream) in gymrl_ddqn_update_args' slots."""

    def __init__(self, net):
        self.fc1, self.fc2, self.fc3 = (net.net[0], net.net[2], net.net[4]) if hasattr(net, "net") else net


def _q_act_args(name, env, net, ring, cap, images):
    if tuple(ring[0].shape[1:]) != (env.obs_dim,) or tuple(ring[1].shape[1:]) != (1,):
        raise ValueError(f"{name}: ring rows {tuple(ring[0].shape)} / {tuple(ring[1].shape)} do not fit the env")
    a = DqnActArgs()
    layers = _Layers3(net)
    _set_act_env(a, env, layers, ring, cap, images)
    _td3_actor_params(a.policy, layers)
    return a


def _q_update_args(make, name, B, D, A, fc1_width, opt, ring, gamma, loss_sum, workspace, td_out=None, set_cap=False):
    """What the value learners' update blocks (gymrl_dqn / ddqn / ndqn_update_args) share: the checks — before the block is made
    (make()) or a network is looked at (fc1_width()) —, the shapes, the ring (set_cap: its row count, where the kernel checks rows
    against it), the policy net's optimiser and the addresses."""
    if loss_sum.dtype != torch.float64 or loss_sum.numel() != 1:
        raise ValueError(f"{name}: loss_sum must be a float64[1]")
    if td_out is not None and (td_out.dtype != torch.float32 or td_out.numel() != B):
        raise ValueError(f"{name}: td_out must be a float32 [{B}]")
    if tuple(ring[0].shape[1:]) != (D,) or tuple(ring[1].shape[1:]) != (1,):
        raise ValueError(f"{name}: ring rows {tuple(ring[0].shape)} / {tuple(ring[1].shape)}, expected [.., {D}] / [.., 1]")
    a = make()
    a.B, a.D, a.A, a.H, a.gamma = B, D, A, fc1_width(), float(gamma)
    if set_cap:
        a.cap = ring[0].shape[0]
    if td_out is not None:
        a.td_out = _addr(td_out)
    _set_ring(a, ring)
    _set_optimisers(a, opt, policy=opt)
    a.loss_sum, a.workspace = _addr(loss_sum), _addr(workspace)
    return a


def dqn_update_workspace(B, D, A, H, device):
    return _zeroed_workspace(lib().gymrl_dqn_update_workspace_bytes(B, D, A, H), device)


def dqn_images(H, device):
    """The three weight images of the H x H layer (gymrl_dqn_update_args.images), or None when H % 16 != 0."""
    return torch.zeros(3 * H * H, device=device) if H % 16 == 0 else None


def dqn_pack_images(a):
    """gymrl_dqn_pack_images: rebuild every image from the parameters as they are now."""
    check(lib().gymrl_dqn_pack_images(C.byref(a), _stream()), "gymrl_dqn_pack_images")


def dqn_act_args(env, policy, ring, cap, images=None):
    """A gymrl_dqn_act_args with everything that does not change from step to step filled in."""
    return _q_act_args("dqn_act_args", env, policy, ring, cap, images)


def dqn_act_step(a, env, obs, obs_out, epsilon=0.0, epsilon_dev=None, cursor=0, cursor_dev=None, u=None, seed=0, counter=0,
                 counter_dev=None, action_out=None, rew_out=None, done_out=None, ep_ret_out=None, ep_stats=None,
                 entry=None):
    """gymrl_dqn_act_step: policy net on obs [N, D], the epsilon-greedy choice (u = f32[N, 2] uniforms or None:
    gymrl_epsilon_greedy's Philox keys under (seed, counter); epsilon rounded to float32 as epsilon_greedy() passes it, or
    epsilon_dev = f32[1] on the device), the env's step with auto-reset (CartPole-v1; MountainCar-v0 and Acrobot-v1 through
    gymrl_dqn_act_step_classic), replay rows at (cursor + env) % cap — ONE launch.  entry: another kernel on the same block."""
    if tuple(obs.shape) != (a.N, a.D) or tuple(obs_out.shape) != (a.N, a.D):
        raise ValueError(f"dqn_act_step: obs {tuple(obs.shape)} / obs_out {tuple(obs_out.shape)}, expected {(a.N, a.D)}")
    if u is not None and (u.dtype != torch.float32 or u.numel() != a.N * 2 or not u.is_contiguous()):
        raise ValueError("dqn_act_step: u must be a contiguous float32 [N, 2]")
    if action_out is not None and (action_out.dtype != torch.int32 or action_out.numel() != a.N):
        raise ValueError("dqn_act_step: action_out must be int32 [N]")
    _set_act_io(a, env, obs, obs_out, cursor, cursor_dev, (action_out, rew_out, done_out, ep_ret_out, ep_stats))
    a.u = _addr(u)
    a.seed, a.counter, a.counter_dev = seed, counter, _addr(counter_dev)
    a.epsilon, a.epsilon_dev = float(epsilon), _addr(epsilon_dev)
    entry = entry or _classic_act_entry("gymrl_dqn_act_step", a.env_kind)
    check(getattr(lib(), entry)(C.byref(a), _stream()), entry)


def dqn_update_args(B, D, A, policy, target, opt, ring, gamma, loss_sum, workspace, images=None):
    """A gymrl_dqn_update_args with the per-trainer constants filled in.  opt: the policy net's FusedAdam (its clamp_abs is the
    update's); loss_sum: f64[1] (sum of td^2)."""
    a = _q_update_args(DqnUpdateArgs, "dqn_update_args", B, D, A, lambda: _Layers3(policy).fc1.weight.shape[0], opt, ring, gamma, loss_sum,
                       workspace)
    _td3_actor_params(a.policy, _Layers3(policy))
    _td3_actor_params(a.target, _Layers3(target))
    a.clamp_abs, a.images = float(opt.clamp_abs), _addr(images)
    return a


def dqn_update(a, idx=None, idx_seed=0, idx_counter=0, idx_size=0, idx_dev=None, adam_policy=None, adam_policy_dev=None):
    """gymrl_dqn_update: dqn_cartpole.DQNTrainer.update() as two launches.  idx: i32[B] rows or None (the keyed draw);
    adam_policy: the 16-byte block of adam_bias() (host) or adam_policy_dev a device view of it."""
    if idx is not None and (idx.dtype != torch.int32 or idx.numel() != a.B):
        raise ValueError(f"dqn_update: idx must be int32 [{a.B}]")
    _set_draw(a, idx, idx_seed, idx_counter, idx_size, idx_dev)
    _set_adam_bias(a, adam_policy=adam_policy)
    a.adam_policy_dev = _addr(adam_policy_dev)
    check(lib().gymrl_dqn_update(C.byref(a), _stream()), "gymrl_dqn_update")


# ------------------------------------------ fused DDQN + PER update step ---
DDQN_FUSED_MAX_BATCH = 256     # one grid of at most 16 slabs in the row phase (ddqn_step.hip kDdqnMaxBatch)


def ddqn_fused_shape_ok(B, D, A, H, dueling=False):
    """Shapes gymrl_ddqn_update takes (include/gymrl.h; the dueling instance: two actions): everything else runs layer by layer."""
    return _fused_shape_ok(B, D, A, H, DDQN_FUSED_MAX_BATCH, 4) and (A == 2 or not dueling)


def ddqn_update_workspace(B, D, A, H, device):
    return _zeroed_workspace(lib().gymrl_ddqn_update_workspace_bytes(B, D, A, H), device)


def ddqn_pack_images(a):
    """gymrl_ddqn_pack_images: rebuild every image (dqn_images' buffer) from the parameters as they are now."""
    check(lib().gymrl_ddqn_pack_images(C.byref(a), _stream()), "gymrl_ddqn_pack_images")


def ddqn_act_args(env, layers, ring, cap, images=None):
    """A gymrl_dqn_act_args for gymrl_dqn_act_step (layers = fc1, fc2, fc3) or gymrl_ddqn_duel_act_step (fc1, value_stream,
    advantage_stream; no images)."""
    return _q_act_args("ddqn_act_args", env, layers, ring, cap, images)


def ddqn_duel_act_step(a, env, obs, obs_out, **kw):
    """gymrl_ddqn_duel_act_step: dqn_act_step's arguments, the dueling network's kernel."""
    dqn_act_step(a, env, obs, obs_out, entry="gymrl_ddqn_duel_act_step", **kw)


def ddqn_update_args(B, D, A, policy_layers, target_layers, opt, ring, gamma, td_out, loss_sum, workspace, images=None, dueling=False):
    """A gymrl_ddqn_update_args with the per-trainer constants filled in.  policy_layers / target_layers: (fc1, fc2, fc3), or
    with dueling (fc1, value_stream, advantage_stream); opt: the policy net's FusedAdam (its clamp_abs is the update's);
    td_out: f32[B]; loss_sum: f64[1] (sum of td^2 * w)."""
    a = _q_update_args(DdqnUpdateArgs, "ddqn_update_args", B, D, A, lambda: _Layers3(policy_layers).fc1.weight.shape[0], opt, ring, gamma,
                       loss_sum, workspace, td_out=td_out, set_cap=True)
    _td3_actor_params(a.policy, _Layers3(policy_layers))
    _td3_actor_params(a.target, _Layers3(target_layers))
    a.dueling, a.clamp_abs, a.images = int(dueling), float(opt.clamp_abs), _addr(None if dueling else images)
    return a


def ddqn_update(a, idx, is_weight, adam_policy=None, adam_policy_dev=None):
    """gymrl_ddqn_update: ddqn_per_cartpole.DDQNPERTrainer.update() between the draw and the tree update, two launches.
    idx: i32[B] ring rows, is_weight: f32[B]; adam_policy: the 16-byte block of adam_bias() (host) or adam_policy_dev a device
    view of it.  A row outside the ring is not read: it counts as a zero row of weight 0."""
    if idx.dtype != torch.int32 or idx.numel() != a.B or is_weight.dtype != torch.float32 or is_weight.numel() != a.B:
        raise ValueError(f"ddqn_update: idx must be int32 [{a.B}] and is_weight float32 [{a.B}]")
    a.idx, a.is_weight = _addr(idx), _addr(is_weight)
    _set_adam_bias(a, adam_policy=adam_policy)
    a.adam_policy_dev = _addr(adam_policy_dev)
    check(lib().gymrl_ddqn_update(C.byref(a), _stream()), "gymrl_ddqn_update")


# --------------------------------------------- fused Rainbow vector step ---
def rainbow_fused_shape_ok(B, D, A, H):
    return _fused_shape_ok(B, D, A, H, FUSED_MAX_BATCH, 3)


def rainbow_update_workspace(B, D, A, H, device):
    # zeroed: the hand-off flags between gymrl_rainbow_update's three workgroups per slab live in it (zero before the first launch, left zero)
    return torch.zeros(int(lib().gymrl_rainbow_update_workspace_bytes(B, D, A, H)), dtype=torch.uint8, device=device)


def rainbow_act_args(env, net, win, ring, cap, n_steps, gamma, max_episode_steps):
    """A gymrl_rainbow_act_args with the per-trainer constants filled in (net: DuelingNoisyNetwork — fc1 / fc2 are read in
    place, the noisy heads arrive per step as gymrl_noisy_combine's stacked output)."""
    a = RainbowActArgs()
    a.N, a.D, a.A, a.H = env.n, env.obs_dim, env.act_dim, net.fc1.weight.shape[0]
    a.env_kind, a.env_state, a.env_id0 = env.kind, _addr(env.state), env.env_id0
    a.fc1_w, a.fc1_b, a.fc2_w, a.fc2_b = _addr(net.fc1.weight), _addr(net.fc1.bias), _addr(net.fc2.weight), _addr(net.fc2.bias)
    a.max_episode_steps = int(max_episode_steps)
    a.w_state, a.w_action, a.w_reward, a.w_next, a.w_terminal, a.w_done = (_addr(t) for t in win)
    a.n_steps, a.gamma = int(n_steps), float(gamma)
    a.r_state, a.r_action, a.r_reward, a.r_next, a.r_flag = (_addr(t) for t in ring)
    a.cap = cap
    return a


def rainbow_act_step(a, env, obs, obs_out, head_w, head_b, pushes=0, cursor=0, push_dev=None, action_out=None, rew_out=None,
                     done_out=None, ep_ret_out=None, ep_stats=None, fc2_img=None):
    """gymrl_rainbow_act_step: greedy acting on the noisy Q + CartPole step + n-step push, one launch.  Returns what
    gymrl_nstep_push returns: whether rows were emitted (by the HOST's push count).  fc2_img: the forward weight image of fc2
    (noisy_combine(images=...)) — the caller vouches that it equals fc2.weight; None: read in place."""
    a.env_seed = env.seed
    a.fc2_img = _addr(fc2_img)
    a.obs, a.obs_out = _ptr(obs, torch.float32).value, _ptr(obs_out, torch.float32).value
    a.head_w, a.head_b = _ptr(head_w, torch.float32).value, _ptr(head_b, torch.float32).value
    a.pushes, a.cursor, a.push_dev = pushes, cursor, _addr(push_dev)
    a.action_out, a.rew_out, a.done_out, a.ep_ret_out, a.ep_stats = (_addr(t) for t in (action_out, rew_out, done_out, ep_ret_out, ep_stats))
    check(lib().gymrl_rainbow_act_step(C.byref(a), _stream()), "gymrl_rainbow_act_step")
    return pushes + 1 >= a.n_steps


def rainbow_update_args(B, D, A, policy, target, ring, gamma_n, loss_sum, d_head_w, d_head_b, workspace):
    a = RainbowUpdateArgs()
    a.B, a.D, a.A, a.H, a.gamma_n = B, D, A, policy.fc1.weight.shape[0], float(gamma_n)
    a.r_state, a.r_action, a.r_reward, a.r_next, a.r_flag = (_addr(t) for t in ring)
    a.p_fc1_w, a.p_fc1_b, a.p_fc2_w, a.p_fc2_b = (_addr(t) for t in (policy.fc1.weight, policy.fc1.bias, policy.fc2.weight, policy.fc2.bias))
    a.t_fc1_w, a.t_fc1_b, a.t_fc2_w, a.t_fc2_b = (_addr(t) for t in (target.fc1.weight, target.fc1.bias, target.fc2.weight, target.fc2.bias))
    a.d_fc1_w, a.d_fc1_b, a.d_fc2_w, a.d_fc2_b = (_addr(t) for t in (policy.fc1.weight.grad, policy.fc1.bias.grad, policy.fc2.weight.grad,
                                                                     policy.fc2.bias.grad))
    a.d_head_w, a.d_head_b, a.loss_sum, a.workspace = _addr(d_head_w), _addr(d_head_b), _addr(loss_sum), _addr(workspace)
    return a


def rainbow_update(a, idx, is_weight, head_w, head_b, td_out, split=None, phase=0, images=None):
    """gymrl_rainbow_update: gather + the three forwards + TD loss gradient + backward chain (rows), every weight gradient
    (tiles) — two launches.  head_w [3 (A+1), H] / head_b [3 (A+1)]: gymrl_noisy_combine's stacked output.
    images: (policy fc2 forward, policy fc2 input-gradient, target fc2 forward) weight images the caller vouches for, or None."""
    a.idx, a.is_weight = _ptr(idx, torch.int32).value, _addr(is_weight)
    a.p_fc2_img_f, a.p_fc2_img_b, a.t_fc2_img_f = (None, None, None) if images is None else (_addr(t) for t in images)
    a.head_w, a.head_b, a.td_out = _ptr(head_w, torch.float32).value, _ptr(head_b, torch.float32).value, _ptr(td_out, torch.float32).value
    # split: [(dw_mu, dw_sigma, db_mu, db_sigma, w_eps, b_eps)] of the advantage and the value layer -> gymrl_noisy_split's work
    # happens in the weight-gradient launch (None: the stacked gradient goes to d_head_w / d_head_b)
    a.split_heads = 0 if split is None else 1
    if split is not None:
        for l, (wm, wsg, bm, bsg, we, be) in enumerate(split):
            a.dw_mu[l], a.dw_sigma[l], a.db_mu[l], a.db_sigma[l] = _addr(wm), _addr(wsg), _addr(bm), _addr(bsg)
            a.w_eps[l], a.b_eps[l] = _addr(we), _addr(be)
    check(lib().gymrl_rainbow_update(C.byref(a), phase, _stream()), "gymrl_rainbow_update")



# ---------------------------------- fused NoisyNet dueling DQN vector step ---
NDQN_FUSED_MAX_BATCH = 256     # one grid of at most 16 slabs in the row phase (noisy_dqn_step.hip kNdqnMaxBatch)
NDQN_LAYERS = ("fc1", "fc2", "value_stream", "advantage_stream")


def ndqn_fused_shape_ok(B, D, A, H):
    """Shapes gymrl_ndqn_combine / _act_step / _update take (include/gymrl.h; two actions: the dueling combine's order is
    pinned for them): everything else runs layer by layer."""
    return _fused_shape_ok(B, D, A, H, NDQN_FUSED_MAX_BATCH, 4) and A == 2


def ndqn_raw_len(D, A, H):
    """Floats of one forward's raw-draw row: per layer the input-side draws, then the output-side ones."""
    return (D + H) + (H + H) + (H + 1) + (H + A)


def ndqn_update_workspace(B, D, A, H, device):
    return _zeroed_workspace(lib().gymrl_ndqn_update_workspace_bytes(B, D, A, H), device)


def _ndqn_params(dst, net):
    for k, name in enumerate(NDQN_LAYERS):
        layer = getattr(net, name)
        dst.w_mu[k], dst.w_sigma[k], dst.b_mu[k], dst.b_sigma[k] = (_addr(t) for t in (layer.weight_mu, layer.weight_sigma, layer.bias_mu,
                                                                                      layer.bias_sigma))


def ndqn_combine_args(D, A, policy, workspace):
    """A gymrl_ndqn_combine_args for `policy` (a NoisyDuelingQNetwork: the layers' own seeds key the draws)."""
    a = NdqnCombineArgs()
    a.D, a.A, a.H = D, A, policy.fc1.out_features
    _ndqn_params(a.policy, policy)
    for k, name in enumerate(NDQN_LAYERS):
        a.seed[k] = getattr(policy, name).seed
    a.workspace = _addr(workspace)
    return a


def ndqn_combine(a, counters=(0, 0, 0), counter_dev=None, raw=(None, None, None)):
    """gymrl_ndqn_combine: the effective parameters of sets C, A, B in one launch.  counters: the three draws' Philox counters
    (or counter_dev = u64[3] on the device); raw: per set a float32 raw row (ndqn_raw_len floats) in place of the draw."""
    n = ndqn_raw_len(a.D, a.A, a.H)
    for k in range(3):
        a.counter[k] = int(counters[k])
        if raw[k] is not None and (raw[k].dtype != torch.float32 or raw[k].numel() != n or not raw[k].is_contiguous()):
            raise ValueError(f"ndqn_combine: raw[{k}] must be a contiguous float32 [{n}]")
        a.raw[k] = _addr(raw[k])
    a.counter_dev = _addr(counter_dev)
    check(lib().gymrl_ndqn_combine(C.byref(a), _stream()), "gymrl_ndqn_combine")


def ndqn_act_args(env, policy, ring, cap, workspace):
    """A gymrl_ndqn_act_args with everything that does not change from step to step filled in."""
    if tuple(ring[0].shape[1:]) != (env.obs_dim,) or tuple(ring[1].shape[1:]) != (1,):
        raise ValueError(f"ndqn_act_args: ring rows {tuple(ring[0].shape)} / {tuple(ring[1].shape)} do not fit the env")
    a = NdqnActArgs()
    a.N, a.D, a.A, a.H = env.n, env.obs_dim, env.act_dim, policy.fc1.out_features
    a.env_kind, a.env_state, a.env_seed, a.env_id0 = env.kind, _addr(env.state), env.seed, env.env_id0
    _set_ring(a, ring)
    a.cap, a.workspace = cap, _addr(workspace)
    return a


def ndqn_act_step(a, env, obs, obs_out, cursor=0, cursor_dev=None, action_out=None, rew_out=None, done_out=None, ep_ret_out=None,
                  ep_stats=None):
    """gymrl_ndqn_act_step: the noisy Q on set C of the last gymrl_ndqn_combine, argmax, CartPole step with auto-reset, replay
    rows at (cursor + env) % cap — ONE launch."""
    if tuple(obs.shape) != (a.N, a.D) or tuple(obs_out.shape) != (a.N, a.D):
        raise ValueError(f"ndqn_act_step: obs {tuple(obs.shape)} / obs_out {tuple(obs_out.shape)}, expected {(a.N, a.D)}")
    if action_out is not None and (action_out.dtype != torch.int32 or action_out.numel() != a.N):
        raise ValueError("ndqn_act_step: action_out must be int32 [N]")
    _set_act_io(a, env, obs, obs_out, cursor, cursor_dev, (action_out, rew_out, done_out, ep_ret_out, ep_stats))
    check(lib().gymrl_ndqn_act_step(C.byref(a), _stream()), "gymrl_ndqn_act_step")


def ndqn_update_args(B, D, A, policy, target, opt, ring, gamma, loss_sum, workspace):
    """A gymrl_ndqn_update_args with the per-trainer constants filled in.  opt: the policy net's FusedAdam; loss_sum: f64[1]."""
    a = _q_update_args(NdqnUpdateArgs, "ndqn_update_args", B, D, A, lambda: policy.fc1.out_features, opt, ring, gamma, loss_sum, workspace,
                       set_cap=True)
    _ndqn_params(a.policy, policy)
    _ndqn_params(a.target, target)
    return a


def ndqn_update(a, idx=None, idx_seed=0, idx_counter=0, idx_size=0, idx_dev=None, adam_policy=None, adam_policy_dev=None):
    """gymrl_ndqn_update: noisy_dqn_cartpole.NoisyDQNTrainer.update() behind a gymrl_ndqn_combine, three launches.  idx: i32[B]
    rows or None (the keyed draw); adam_policy: the 16-byte block of adam_bias() (host) or adam_policy_dev a device view of it."""
    if idx is not None and (idx.dtype != torch.int32 or idx.numel() != a.B):
        raise ValueError(f"ndqn_update: idx must be int32 [{a.B}]")
    _set_draw(a, idx, idx_seed, idx_counter, idx_size, idx_dev)
    _set_adam_bias(a, adam_policy=adam_policy)
    a.adam_policy_dev = _addr(adam_policy_dev)
    check(lib().gymrl_ndqn_update(C.byref(a), _stream()), "gymrl_ndqn_update")

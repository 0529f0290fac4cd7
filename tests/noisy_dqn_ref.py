"""NoisyNet dueling DQN (noisy_dqn_cartpole.py) restated in numpy float32: the factorised noise, the four-layer forward, the
double-Q update with its hand-written backward, and Adam.  No torch, no GPU: tests/test_noisy_dqn_golden.py holds it to the
golden recorded from the reference, and the GPU tests hold the kernels to the same golden.

A parameter set is a dict with the reference's state-dict keys (`fc1.weight_mu`, ...).  Raw draws travel as ONE float32 row
per training-mode forward: for each layer in the forward's order (fc1, fc2, value_stream, advantage_stream) the input-side
N(0, 1) vector, then the output-side one — the order NoisyLinear.reset_noise draws them in.
"""
import numpy as np

LAYERS = ("fc1", "fc2", "value_stream", "advantage_stream")
F32 = np.float32


def layer_dims(D, H, A):
    """(in, out) of the four layers."""
    return ((D, H), (H, H), (H, 1), (H, A))


def raw_len(D, H, A):
    return sum(i + o for i, o in layer_dims(D, H, A))


def scale_noise(x):
    """f(x) = sign(x) sqrt(|x|)."""
    x = np.asarray(x, F32)
    return (np.sign(x) * np.sqrt(np.abs(x))).astype(F32)


def split_raw(raw, D, H, A):
    """One forward's raw row -> [(eps_in, eps_out)] per layer, scaled."""
    out, o = [], 0
    for i, n in layer_dims(D, H, A):
        out.append((scale_noise(raw[o:o + i]), scale_noise(raw[o + i:o + i + n])))
        o += i + n
    return out


def effective(p, eps=None):
    """[(W, b)] per layer: mu + sigma * eps (eps = split_raw's list), or mu alone (eval mode)."""
    out = []
    for k, name in enumerate(LAYERS):
        W, b = p[name + ".weight_mu"].astype(F32), p[name + ".bias_mu"].astype(F32)
        if eps is not None:
            ei, eo = eps[k]
            W = W + p[name + ".weight_sigma"].astype(F32) * np.outer(eo, ei).astype(F32)
            b = b + p[name + ".bias_sigma"].astype(F32) * eo
        out.append((W.astype(F32), b.astype(F32)))
    return out


def forward(eff, x):
    """-> (q, cache) for x [B, D]."""
    (W1, b1), (W2, b2), (Wv, bv), (Wa, ba) = eff
    h1 = np.maximum(x @ W1.T + b1, F32(0))
    h2 = np.maximum(h1 @ W2.T + b2, F32(0))
    v, a = h2 @ Wv.T + bv, h2 @ Wa.T + ba
    q = v + (a - a.mean(axis=-1, keepdims=True, dtype=F32))
    return q.astype(F32), (x, h1, h2)


def dims_of(p):
    H, D = p["fc1.weight_mu"].shape
    return D, H, p["advantage_stream.weight_mu"].shape[0]


def select_action(p, state, raw=None):
    """argmax of the noisy Q (raw: one forward's draws) or of the mu-only Q (raw None); first maximum wins.  -> (action, q)."""
    eps = None if raw is None else split_raw(raw, *dims_of(p))
    q, _ = forward(effective(p, eps), np.asarray(state, F32).reshape(1, -1))
    return int(np.argmax(q[0])), q[0]


def new_adam(p):
    return {"t": 0, "m": {k: np.zeros_like(v, F32) for k, v in p.items() if _trainable(k)},
            "v": {k: np.zeros_like(v, F32) for k, v in p.items() if _trainable(k)}}


def _trainable(k):
    return k.endswith(("_mu", "_sigma"))


def update(p, target, adam, batch, raw_a, raw_b, gamma, lr, beta1=0.9, beta2=0.999, eps_adam=1e-8):
    """One update() (:217-257) in place on p and adam.  batch = (states, actions, rewards, next_states, dones); raw_a: the draws
    of policy_net(states) — the gradient flows through them —, raw_b: those of policy_net(next_states).  -> (loss, q_mean)."""
    s, act, r, s2, d = batch
    s, s2, r, d = np.asarray(s, F32), np.asarray(s2, F32), np.asarray(r, F32), np.asarray(d, F32)
    act = np.asarray(act, np.int64)
    B = s.shape[0]
    D, H, A = dims_of(p)
    eps_a = split_raw(raw_a, D, H, A)
    eff_a = effective(p, eps_a)
    q, (x, h1, h2) = forward(eff_a, s)
    q_online, _ = forward(effective(p, split_raw(raw_b, D, H, A)), s2)
    q_target, _ = forward(effective(target), s2)
    rows = np.arange(B)
    astar = np.argmax(q_online, axis=1)
    y = (r + F32(gamma) * q_target[rows, astar] * (F32(1) - d)).astype(F32)
    qa = q[rows, act]
    td = (qa - y).astype(F32)
    loss = float(np.mean(td.astype(np.float64) ** 2))
    dq = np.zeros((B, A), F32)
    dq[rows, act] = F32(2) * td / F32(B)
    # the dueling combine's backward, then the chain
    dv = dq.sum(axis=1, keepdims=True, dtype=F32)
    da = (dq - dq.mean(axis=1, keepdims=True, dtype=F32)).astype(F32)
    (W1, _), (W2, _), (Wv, _), (Wa, _) = eff_a
    dh2 = dv @ Wv + da @ Wa
    dz2 = (dh2 * (h2 > 0)).astype(F32)
    dz1 = ((dz2 @ W2) * (h1 > 0)).astype(F32)
    grads_eff = [(dz1.T @ x, dz1.sum(0)), (dz2.T @ h1, dz2.sum(0)), (dv.T @ h2, dv.sum(0)), (da.T @ h2, da.sum(0))]
    grads = {}
    for name, (gW, gb), (ei, eo) in zip(LAYERS, grads_eff, eps_a):
        gW, gb = gW.astype(F32), gb.astype(F32)
        grads[name + ".weight_mu"], grads[name + ".weight_sigma"] = gW, gW * np.outer(eo, ei).astype(F32)
        grads[name + ".bias_mu"], grads[name + ".bias_sigma"] = gb, gb * eo
    adam_step(p, grads, adam, lr, beta1, beta2, eps_adam)
    return loss, float(np.mean(qa.astype(np.float64)))


def adam_step(p, grads, adam, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """torch.optim.Adam's step in float32 (bias corrections as host doubles)."""
    adam["t"] += 1
    t = adam["t"]
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    step_size, bc2_sqrt = F32(lr / bc1), F32(np.sqrt(bc2))
    for k, g in grads.items():
        g = g.astype(F32)
        m = adam["m"][k] = (adam["m"][k] + (g - adam["m"][k]) * F32(1.0 - beta1)).astype(F32)
        v = adam["v"][k] = (adam["v"][k] * F32(beta2) + F32(1.0 - beta2) * g * g).astype(F32)
        denom = np.sqrt(v) / bc2_sqrt + F32(eps)
        p[k] = (p[k] - step_size * (m / denom)).astype(F32)

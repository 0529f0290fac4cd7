"""Phasic Policy Gradient with a GRU (PSCN -> MLPRNN -> actor / critic / aux-critic heads, whole-episode recurrent updates,
dual-clip policy phase + aux phase with clone loss) — MI355X engine behind the reference's
algorithms/ppg_rnn_lunarlander.py surface: Config :35-56, MLP :67-89, PSCN :92-122, MLPRNN :125-140, ActorCriticPPG
:143-176, EpisodeBuffer :179-236, PPGTrainer :285-547 (choose_action :311-320, evaluate_action :322-328, update :330-407,
save_model / load_model :409-429, train :431-499, eval :501-524, test :526-547).  ppo_rnn_lunarlander.py is the same file
without the aux head and the aux phase; `gymrl_amd.ppo_rnn_lunarlander` builds on this module.

What runs where: acting — the whole network's single step plus the Categorical draw — is ONE launch per vector step
(`gymrl_mlprnn_act`); env stepping, observation / reward normalisation (masked to the live envs), per-episode GAE
(`gymrl_episode_gae`), the GRU over whole episodes (`gymrl_gru_seq_fwd/_bwd` behind `_GRUSeq`), the L5 / L6 losses and
clip-norm + Adam are HIP kernels; the dense layers of the update are PyTorch-ROCm library GEMMs.  Parameter names are the
reference's (`fc_head.layers.0.mlp.1.weight`, `rnn.rnn.weight_hh_l0`, ...), so its state_dicts load unchanged.

Vectorisation by rounds: a round resets all N envs and steps them until every env's episode has ended; a finished env is
masked (it stores nothing and does not touch the running statistics).  Round r, env i is episode r*N + i.  With N = 1 and
episodes_per_minibatch = 1 this is the reference's loop.

Adam parity: torch's zero_grad() sets grads to None and Adam.step skips such parameters, so the policy phase does not step
aux_critic_fc and the aux phase does not step critic_fc (their moments do not decay, their step counts do not advance).
The flat buffer is laid out critic | trunk + actor | aux, each phase's parameters form one contiguous range, and every
sub-range is stepped with its own step count under the phase's shared clip norm.
"""
import os
from collections import deque

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .envs import VecEnv
from .flat import GradSink, flatten_module
from .utils.normalization import Normalization, RewardScaling


class Config:
    def __init__(self):
        self.env_name = "LunarLander-v3"
        self.seed = None
        self.max_episodes = 5000
        self.max_steps = 20000
        self.batch_size = 4
        self.epochs = 10
        self.aux_epochs = 6
        self.clip = 0.2
        self.dual_clip = 3.0
        self.gamma = 0.995
        self.lamda = 0.95
        self.val_coef = 0.5
        self.ent_coef = 1e-2
        self.beta_clone = 1.0
        self.lr = 1e-3
        self.grad_clip = 0.5
        self.eval_freq = 10
        self.save_freq = 50
        self.device = "cuda"
        self.save_path = "./checkpoints/PPG_RNN_LunarLander.pth"
        # --- vectorised-engine additions ---
        self.num_envs = 1                  # envs stepped together; one round = one episode of each
        self.episodes_per_minibatch = 1    # G episodes per optimiser step (loss = mean over episodes); 1 = the reference
        self.fused_eval = False            # LunarLander: eval() as ONE launch (gymrl_lunar_mlprnn_eval) on the loop's own streams
        self.fused_collect = False         # LunarLander, num_envs <= 16: a collection round as ONE launch (gymrl_lunar_mlprnn_collect)


def initialize_weights(layer):
    if isinstance(layer, nn.Linear):
        nn.init.kaiming_uniform_(layer.weight, nonlinearity="leaky_relu")
        if layer.bias is not None:
            nn.init.constant_(layer.bias, 0)
    return layer


class MLP(nn.Module):
    """:67-89 — ONE nn.PReLU shared by all activations of the MLP."""

    def __init__(self, dim_list, activation=None, last_act=False):
        super().__init__()
        if activation is None:
            activation = nn.PReLU()
        layers = []
        for i in range(len(dim_list) - 1):
            layers.append(initialize_weights(nn.Linear(dim_list[i], dim_list[i + 1])))
            if i < len(dim_list) - 2:
                layers.append(activation)
        if last_act:
            layers.append(activation)
        self.mlp = nn.Sequential(*layers)

    def forward(self, x):
        return self.mlp(x)


class PSCN(nn.Module):
    """:92-122 — each layer keeps its first half and feeds its second half on."""

    def __init__(self, input_dim, output_dim, depth=4):
        super().__init__()
        min_dim = 2 ** (depth - 1)
        assert output_dim >= min_dim and output_dim % min_dim == 0
        self.layers = nn.ModuleList()
        self.output_dim = output_dim
        in_dim, out_dim = input_dim, output_dim
        for _ in range(depth):
            self.layers.append(MLP([in_dim, out_dim], last_act=True))
            in_dim = out_dim // 2
            out_dim //= 2

    def forward(self, x):
        parts = []
        for i, layer in enumerate(self.layers):
            x = layer(x)
            if i < len(self.layers) - 1:
                split = int(self.output_dim // (2 ** (i + 1)))
                part, x = torch.split(x, [split, split], dim=-1)
                parts.append(part)
            else:
                parts.append(x)
        return torch.cat(parts, dim=-1)


class MLPRNN(nn.Module):
    """:125-140 — cat(rnn_linear(x), GRU(x, h)); rnn_linear has no activation."""

    def __init__(self, input_dim, output_dim, batch_first=True):
        super().__init__()
        assert output_dim % 4 == 0
        self.rnn_size = output_dim // 4
        self.rnn_linear = MLP([input_dim, 3 * self.rnn_size])
        self.rnn = nn.GRU(input_dim, self.rnn_size, batch_first=batch_first)

    def forward(self, x, rnn_state):
        out, rnn_state = self.rnn(x, rnn_state)
        return torch.cat([self.rnn_linear(x), out], dim=-1), rnn_state


class _GRUSeq(torch.autograd.Function):
    """h_seq [Tmax, G, H] = the GRU over G zero-started episodes (time-major, zero padding past each length) on
    gymrl_gru_seq_fwd / _bwd.  dW_hh = sum_t dgh_t^T h_{t-1} and db_hh = sum_t dgh_t are library GEMMs / reductions over
    the flattened rows (padded rows have dgh = 0); dgi flows back into the W_ih GEMM."""

    @staticmethod
    def forward(ctx, gi, W_hh, b_hh, lengths):
        gi = gi.contiguous()
        h_seq, _ = ops.gru_seq_fwd(gi, W_hh.detach(), b_hh.detach(), lengths)
        ctx.save_for_backward(gi, W_hh, b_hh, h_seq)
        ctx.lengths = lengths
        return h_seq

    @staticmethod
    def backward(ctx, d_hseq):
        gi, W_hh, b_hh, h_seq = ctx.saved_tensors
        dgi, dgh, _ = ops.gru_seq_bwd(gi, W_hh.detach(), b_hh.detach(), h_seq, ctx.lengths, d_hseq=d_hseq.contiguous(),
                                      need_dh0=False)
        T, G, H = h_seq.shape
        h_prev = torch.cat([h_seq.new_zeros(1, G, H), h_seq[:-1]], 0).reshape(T * G, H)
        dgh = dgh.reshape(T * G, 3 * H)
        return dgi, dgh.t() @ h_prev, dgh.sum(0), None


class _Episodes:
    """Index maps between flat episode-major rows (episode g = rows [off[g], off[g+1])) and the time-major padded
    [Tmax, G] layout of the sequence kernels (padding reads row M of the source, an appended zero row)."""

    def __init__(self, lengths, device):
        self.lengths = [int(n) for n in lengths]
        G, M = len(self.lengths), sum(self.lengths)
        self.G, self.M, self.T = G, M, max(self.lengths)
        off = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int64)
        self.offsets = off.tolist()
        pack = np.full((self.T, G), M, dtype=np.int64)
        unpack = np.empty(M, dtype=np.int64)
        for g, n in enumerate(self.lengths):
            pack[:n, g] = np.arange(off[g], off[g] + n)
            unpack[off[g]:off[g] + n] = np.arange(n) * G + g
        self.pack = torch.from_numpy(pack.reshape(-1)).to(device)
        self.unpack = torch.from_numpy(unpack).to(device)

    def to_time_major(self, x):
        return torch.cat([x, x.new_zeros(1, x.shape[1])], 0).index_select(0, self.pack).view(self.T, self.G, -1)

    def to_flat(self, x):
        return x.reshape(self.T * self.G, -1).index_select(0, self.unpack)


class ActorCriticPPG(nn.Module):
    """:143-176.  forward() is the reference's torch composition (one unbatched sequence, hidden state carried in rnn_h):
    the tests' comparison.  Training acts through gymrl_mlprnn_act and updates through episodes_forward()."""
    has_aux = True

    def __init__(self, state_dim, action_dim, hidden_size=64):
        super().__init__()
        self.hidden_size = hidden_size
        self.rnn_h = None
        self.fc_head = PSCN(state_dim, 256)
        self.rnn = MLPRNN(256, 256, batch_first=True)
        self.actor_fc = MLP([256, 64, action_dim])
        self.critic_fc = MLP([256, 32, 1])
        if self.has_aux:
            self.aux_critic_fc = MLP([256, 32, 1])

    def reset_hidden(self, device=None):
        if device is None:
            device = next(self.parameters()).device
        self.rnn_h = torch.zeros(1, self.hidden_size, device=device, dtype=torch.float)

    def forward(self, s):
        if self.rnn_h is None:
            self.reset_hidden(s.device)
        x = self.fc_head(s)
        out, self.rnn_h = self.rnn(x, self.rnn_h)
        prob = F.softmax(self.actor_fc(out), dim=-1)
        value = self.critic_fc(out)
        if not self.has_aux:
            return prob, value
        return prob, value, self.aux_critic_fc(out)

    def episodes_forward(self, states, eps, aux=False):
        """states f32[M, D] of G episodes stored back to back, each from h = 0 -> (logits [M, A], value or aux value [M])."""
        x = self.fc_head(states)
        g = self.rnn.rnn
        gi = eps.to_time_major(F.linear(x, g.weight_ih_l0, g.bias_ih_l0))
        h = eps.to_flat(_GRUSeq.apply(gi, g.weight_hh_l0, g.bias_hh_l0, eps.lengths))
        out = torch.cat([self.rnn.rnn_linear(x), h], dim=-1)
        head = self.aux_critic_fc if aux else self.critic_fc
        return self.actor_fc(out), head(out).view(-1)


class RangeAdam:
    """torch.optim.Adam(lr, eps=1e-5) + clip_grad_norm_ over named contiguous ranges of one flat buffer, each range with
    its own step count (a range whose parameters had no gradient in a step is not stepped, as torch skips grad-None
    parameters).  step(names): the clip norm is taken over the union of the named ranges (contiguous), then
    gymrl_adam_step runs per range under that shared norm."""

    def __init__(self, flat_params, flat_grads, ranges, lr, eps, max_grad_norm):
        self.p, self.g = flat_params, flat_grads
        self.ranges = dict(ranges)
        self.m, self.v = torch.zeros_like(flat_params), torch.zeros_like(flat_params)
        self.steps = {k: 0 for k in self.ranges}
        self.param_groups = [dict(lr=lr, betas=(0.9, 0.999), eps=eps)]
        self.max_grad_norm = float(max_grad_norm)
        self._sq = torch.zeros(1, dtype=torch.float64, device=flat_params.device)
        self._ws = ops.reduce_workspace(flat_params.device)

    def step(self, names):
        lo = min(self.ranges[k][0] for k in names)
        hi = max(self.ranges[k][1] for k in names)
        if sum(self.ranges[k][1] - self.ranges[k][0] for k in names) != hi - lo:
            raise ValueError(f"ranges {names} are not contiguous")
        ops.sqnorm(self.g[lo:hi], self._sq, self._ws)
        g = self.param_groups[0]
        for k in names:
            a, b = self.ranges[k]
            self.steps[k] += 1
            ops.adam_step(self.p[a:b], self.g[a:b], self.m[a:b], self.v[a:b], g["lr"], g["betas"][0], g["betas"][1], g["eps"],
                          self.steps[k], max_grad_norm=self.max_grad_norm, sqnorm_buf=self._sq, zero_grad=True)


class PPGTrainer:
    net_cls = ActorCriticPPG

    def __init__(self, config):
        self.cfg = config
        if not torch.cuda.is_available() or not ops.device_ok():
            raise RuntimeError("gymrl_amd PPG-RNN needs an MI355X and libgymrl_hip.so; no CPU fallback")
        N, B, G = int(config.num_envs), int(config.batch_size), int(getattr(config, "episodes_per_minibatch", 1))
        if N < 1 or B % N:
            raise ValueError(f"batch_size ({B}) must be a multiple of num_envs ({N})")
        if G < 1 or B % G:
            raise ValueError(f"batch_size ({B}) must be a multiple of episodes_per_minibatch ({G})")
        if getattr(config, "fused_collect", False) and N > ops.LUNAR_COLLECT_MAX_ENVS:
            raise ValueError(f"fused_collect plays a round in one workgroup: num_envs ({N}) must be at most "
                             f"{ops.LUNAR_COLLECT_MAX_ENVS}")
        self.N, self.G = N, G
        self.device = torch.device(config.device if ":" in str(config.device) else f"cuda:{torch.cuda.current_device()}")
        self.base_seed = 0 if config.seed is None else int(config.seed)
        self.env = VecEnv(self._env_name(), N, device=self.device, seed=self.base_seed)
        self.state_dim, self.action_dim = self.env.observation_space.shape[0], self.env.action_space.n
        g = torch.random.get_rng_state()
        torch.manual_seed(self.base_seed)
        self.net = self.net_cls(self.state_dim, self.action_dim, hidden_size=64)
        torch.random.set_rng_state(g)
        named = [n for n, _ in self.net.named_parameters()]
        critic = [n for n in named if n.startswith("critic_fc.")]
        aux = [n for n in named if n.startswith("aux_critic_fc.")]
        trunk = [n for n in named if n not in critic and n not in aux]
        self.flat_params, self.flat_grads = flatten_module(self.net, self.device, order=critic + trunk + aux)
        params = dict(self.net.named_parameters())

        def span(names):
            offs = [(params[n].data_ptr() - self.flat_params.data_ptr()) // 4 for n in names]
            last = max(range(len(names)), key=lambda i: offs[i])
            end = offs[last] + (params[names[last]].numel() + 63) // 64 * 64
            return min(offs), end

        ranges = {"critic": span(critic), "trunk": span(trunk)}
        if aux:
            ranges["aux"] = span(aux)
        self._group_of = {n: ("critic" if n in critic else "aux" if n in aux else "trunk") for n in named}
        self.optimizer = RangeAdam(self.flat_params, self.flat_grads, ranges, lr=config.lr, eps=1e-5,
                                   max_grad_norm=config.grad_clip)
        self._act_params = ops.mlprnn_params(self.net)
        self._sink = GradSink(self.net)
        self.state_norm = Normalization(self.state_dim, device=self.device)
        self.reward_scaler = RewardScaling(1, config.gamma, num_envs=N, device=self.device)
        self.learn_step = 0
        self.episode_rewards = deque(maxlen=100)
        self.round_count = 0
        self._batch = []                   # compacted rounds of the batch being collected
        self.last_lengths = []             # episode lengths of the last round (host)
        self._parity_noise = None          # tests: callable(round, t) -> f32[N, A] Exp(1) draws, or None
        self._parity_perms = None          # tests: iterator of permutations of range(batch_size), one per epoch
        self.grad_norms = None             # tests: set to [] to record the pre-clip gradient norm of every optimiser step
        d = os.path.dirname(config.save_path)
        if d:
            os.makedirs(d, exist_ok=True)
        print(f"Device: {self.device}")
        print(f"State dim: {self.state_dim}, Action dim: {self.action_dim}")

    def _env_name(self):
        return self.cfg.env_name

    # ---------------------------------------------------------------- acting ---
    @torch.no_grad()
    def choose_action(self, state, hidden=None, live=None, deterministic=False, counter=0, noise_exp=None,
                      probs_out=None):
        """:311-320: one gymrl_mlprnn_act launch.  As in the reference, the hidden state is carried across calls in
        net.rnn_h (net.reset_hidden() zeroes it) unless `hidden` f32[N, 64] is given; either is advanced in place.
        state: one observation [D] -> (action int, log_prob float, value float), the reference's return; N rows [N, D]
        -> (action i32[N], log_prob f32[N], value f32[N]) device tensors."""
        single = np.ndim(state) == 1
        state = torch.as_tensor(state, dtype=torch.float32, device=self.device).reshape(-1, self.state_dim).contiguous()
        if hidden is None:
            h = self.net.rnn_h
            if h is None or tuple(h.shape) != (state.shape[0], 64) or h.device != state.device:
                self.net.rnn_h = torch.zeros(state.shape[0], 64, device=self.device)
            hidden = self.net.rnn_h
        act, logp, value, _, _ = ops.mlprnn_act(state, hidden, self._act_params, self.action_dim, live=live,
                                                noise_exp=noise_exp, seed=self.env.seed, counter=counter,
                                                env_id0=self.env.env_id0, deterministic=deterministic, h_out=hidden,
                                                probs_out=probs_out)
        if single:
            return int(act.item()), float(logp.item()), float(value.item())
        return act, logp, value

    @torch.no_grad()
    def evaluate_action(self, state, hidden=None, live=None):
        """:322-328: argmax of probs (first maximum), the hidden state carried as in choose_action."""
        return self.choose_action(state, hidden, live=live, deterministic=True)[0]

    # ------------------------------------------------------------- collection ---
    @torch.no_grad()
    def collect_round(self):
        """One round: every env plays one episode (:434-471 for N envs).  Appends the compacted episodes to the batch
        and returns their raw returns and lengths (host lists, env order).  With Config.fused_collect the step loop below is
        ONE launch (gymrl_lunar_mlprnn_collect, csrc/collect_lunar_rnn.hip) that writes the same slabs, statistics and returns
        bit for bit; the loop runs whenever the launch cannot play the round (explicit noise, another env).  self.env is not
        stepped by the launch: every round starts with a reset, so nothing reads its state."""
        cfg, env, N, D, dev = self.cfg, self.env, self.N, self.state_dim, self.device
        # `for step in range(cfg.max_steps)` (:445): a round stops storing an env's episode after max_steps steps.  Every
        # round starts with a real reset of every env, so no cut episode has to be abandoned inside the stepper
        # (VecEnv.abandon) — the next round starts fresh envs anyway.
        Tcap = max(1, min(int(cfg.max_steps), int(env.max_steps)))
        z = lambda *s, **k: torch.zeros(*s, device=dev, **k)   # noqa: E731
        states, live = z(Tcap + 1, N, D), z(Tcap + 1, N, dtype=torch.uint8)
        act, logp, value = z(Tcap + 1, N, dtype=torch.int32), z(Tcap + 1, N), z(Tcap + 1, N)
        rew, done, dw = z(Tcap, N), z(Tcap, N, dtype=torch.uint8), z(Tcap, N, dtype=torch.uint8)
        raw_obs, term_obs, raw_rew = z(N, D), z(N, D), z(N)
        terminated, truncated = z(N, dtype=torch.uint8), z(N, dtype=torch.uint8)
        ep_ret = z(N)
        seed = self.base_seed if cfg.seed is not None else self.base_seed + 0x9E3779B1 * (self.round_count + 1)
        c0 = self.round_count * (Tcap + 1)
        if getattr(cfg, "fused_collect", False) and self._parity_noise is None and self._eval_fusable():
            env.seed = seed & 0x7FFFFFFFFFFFFFFF               # what reset(seed=...) leaves: choose_action() draws under it
            self.reward_scaler.reset()
            slabs = dict(states=states, act=act, logp=logp, value=value, rew=rew, done=done, dw=dw, live=live, ep_ret=ep_ret,
                         lengths=z(N, dtype=torch.int32))
            ops.lunar_mlprnn_collect(self._act_params, N, Tcap, env.seed, env.env_id0, c0, self.state_norm.running_ms.stats,
                                     self.reward_scaler.running_ms.stats, self.reward_scaler.R, cfg.gamma, out=slabs)
            lengths = slabs["lengths"].cpu().numpy().astype(np.int64)
            return self._compact(int(lengths.max()), lengths, ep_ret, states, act, rew, done, dw, logp, value)
        env.reset(raw_obs, seed=seed & 0x7FFFFFFFFFFFFFFF)
        self.reward_scaler.reset()
        hidden = z(N, 64)
        live[0].fill_(1)
        noise = (lambda t: self._parity_noise(self.round_count, t)) if self._parity_noise is not None else (lambda t: None)
        ops.running_norm_masked(raw_obs, live[0], self.state_norm.running_ms.stats, out=states[0])
        self._act(states[0], hidden, live[0], c0, noise(0), act[0], logp[0], value[0])
        K, t = 16, 0
        while t < Tcap:
            env.step(act[t], raw_obs, raw_rew, term_obs_out=term_obs, terminated_out=terminated, truncated_out=truncated)
            torch.bitwise_or(terminated, truncated, out=done[t])
            dw[t].copy_(terminated)
            ep_ret.add_(raw_rew * live[t])
            ops.running_norm_masked(term_obs, live[t], self.state_norm.running_ms.stats, out=states[t + 1])
            ops.reward_scaling_masked(raw_rew, live[t], cfg.gamma, self.reward_scaler.R, self.reward_scaler.running_ms.stats,
                                      out=rew[t])
            # next_value: the forward on the next (possibly terminal) state with the hidden state carried (:452)
            self._act(states[t + 1], hidden, live[t], c0 + t + 1, noise(t + 1), act[t + 1], logp[t + 1], value[t + 1])
            torch.mul(live[t], 1 - done[t], out=live[t + 1])
            t += 1
            if t % K == 0 and not bool(live[t].any()):
                break
        lengths = live[:t].cpu().numpy().astype(bool).sum(0).astype(np.int64)
        return self._compact(t, lengths, ep_ret, states, act, rew, done, dw, logp, value)

    def _compact(self, T, lengths, ep_ret, states, act, rew, done, dw, logp, value):
        """The round's [T, N] slabs -> the episode-major chunk of the batch; returns the raw returns and the lengths."""
        N, dev = self.N, self.device
        idx = np.concatenate([np.arange(n) * N + i for i, n in enumerate(lengths)])
        sel = torch.from_numpy(idx).to(dev)                  # row (t, i) of the [T, N] slabs, episode-major
        flat = lambda x, t0=0: x[t0:T + t0].reshape(T * N, *x.shape[2:]).index_select(0, sel)   # noqa: E731
        chunk = dict(states=flat(states), act=flat(act), rew=flat(rew), done=flat(done), dw=flat(dw), logp=flat(logp),
                     value=flat(value), next_value=flat(value, 1), lengths=lengths.tolist())
        self._batch.append(chunk)
        self.round_count += 1
        self.last_lengths = lengths.tolist()
        return ep_ret.cpu().tolist(), lengths.tolist()

    def _act(self, s, hidden, live, counter, noise, act_out, logp_out, value_out):
        ops.mlprnn_act(s, hidden, self._act_params, self.action_dim, live=live, noise_exp=noise, seed=self.env.seed,
                       counter=counter, env_id0=self.env.env_id0, h_out=hidden, act_out=act_out, logp_out=logp_out,
                       value_out=value_out)

    # ------------------------------------------------------------------ update ---
    def sample(self):
        """The stored batch (batch_size episodes back to back) with EpisodeBuffer.sample()'s advantages (:217-236), once
        per update."""
        parts = self._batch
        cat = lambda k: torch.cat([p[k] for p in parts])   # noqa: E731
        b = {k: cat(k) for k in ("states", "act", "rew", "done", "dw", "logp", "value", "next_value")}
        b["lengths"] = [n for p in parts for n in p["lengths"]]
        b["offsets"] = np.concatenate([[0], np.cumsum(b["lengths"])]).astype(np.int64).tolist()
        b["adv"], b["v_target"], _ = ops.episode_gae(b["rew"], b["value"], b["next_value"], b["done"], b["dw"], b["offsets"],
                                                     self.cfg.gamma, self.cfg.lamda)
        return b

    def _minibatch(self, b, episodes):
        lens = [b["lengths"][e] for e in episodes]
        rows = torch.from_numpy(np.concatenate([np.arange(b["offsets"][e], b["offsets"][e + 1]) for e in episodes])).to(self.device)
        eps = _Episodes(lens, self.device)
        pick = lambda k: b[k].index_select(0, rows)   # noqa: E731
        return eps, pick("states"), pick("act"), pick("logp"), pick("adv"), pick("v_target")

    def _perm(self):
        if self._parity_perms is not None:
            return np.asarray(next(self._parity_perms), dtype=np.int64)
        return np.random.permutation(self.cfg.batch_size)

    def _opt_step(self, names):
        self.optimizer.step(names)
        if self.grad_norms is not None:
            self.grad_norms.append(float(self.optimizer._sq.sqrt().item()))

    def update(self):
        """:330-407 (PPG) — policy phase, then the aux phase.  Returns the reference's metrics dict."""
        cfg, G = self.cfg, self.G
        b = self.sample()
        self.last_sample = b
        pol = torch.zeros(5, dtype=torch.float64, device=self.device)
        n_pol = 0
        for _ in range(cfg.epochs):
            perm = self._perm()
            for j in range(0, cfg.batch_size, G):
                eps, s, a, lp, adv, vt = self._minibatch(b, perm[j:j + G])
                logits, value = self.net.episodes_forward(s, eps)
                dlogits, dvalue, _ = ops.ppg_policy_loss_fwd_bwd(logits.detach(), value.detach(), a, lp, adv, vt, eps.offsets,
                                                                 cfg.clip, cfg.dual_clip, cfg.val_coef, cfg.ent_coef,
                                                                 metrics_sum=pol)
                self._sink.arm()
                torch.autograd.backward([logits, value], [dlogits, dvalue])
                self._sink.collect()
                self._opt_step(["critic", "trunk"])
                n_pol += 1
        aux = torch.zeros(3, dtype=torch.float64, device=self.device)
        n_aux = 0
        if self.net.has_aux:
            for _ in range(cfg.aux_epochs):
                perm = self._perm()
                for j in range(0, cfg.batch_size, G):
                    eps, s, a, lp, _, vt = self._minibatch(b, perm[j:j + G])
                    logits, aux_value = self.net.episodes_forward(s, eps, aux=True)
                    dlogits, daux, _ = ops.ppg_aux_loss_fwd_bwd(logits.detach(), aux_value.detach(), a, lp, vt, eps.offsets,
                                                                cfg.beta_clone, metrics_sum=aux)
                    self._sink.arm()
                    torch.autograd.backward([logits, aux_value], [dlogits, daux])
                    self._sink.collect()
                    self._opt_step(["trunk", "aux"])
                    n_aux += 1
        self._batch = []
        self.learn_step += 1
        m = (pol / max(n_pol, 1)).tolist()
        out = {"total_loss": m[0], "clip_loss": m[1], "value_loss": m[2], "entropy_loss": m[3], "advantage": m[4]}
        if self.net.has_aux:
            out["aux_value_loss"] = float(aux[0].item()) / max(n_aux, 1)
        out["lr"] = self.optimizer.param_groups[0]["lr"]
        return out

    # -------------------------------------------------------------- checkpoint ---
    def param_steps(self):
        """Adam step count of every parameter, in net.parameters() order."""
        return [self.optimizer.steps[self._group_of[n]] for n, _ in self.net.named_parameters()]

    def save_model(self):
        """:409-417 — net_state_dict, optimizer_state_dict (torch.optim.Adam layout, per-parameter steps), learn_step,
        state_norm (the running statistics; the reference pickles the object), the reward scaler's statistics and the round count
        (so that a resumed run continues the draws and env starts instead of replaying them)."""
        from .utils.checkpoint import adam_state_dict
        state = {"net_state_dict": {k: v.detach().cpu() for k, v in self.net.state_dict().items()},
                 "optimizer_state_dict": adam_state_dict(self.net, self.optimizer, steps=self.param_steps()),
                 "learn_step": self.learn_step,
                 "state_norm": self.state_norm.state_dict(),
                 "reward_scaling": self.reward_scaler.state_dict(),
                 "round_count": self.round_count}
        torch.save(state, self.cfg.save_path)
        print(f"Model saved to {self.cfg.save_path}")

    def load_model(self):
        """:419-429."""
        from .utils.checkpoint import load_adam_state_dict
        if not os.path.exists(self.cfg.save_path):
            print(f"No checkpoint found at {self.cfg.save_path}")
            return
        ck = torch.load(self.cfg.save_path, map_location="cpu", weights_only=False)
        with torch.no_grad():
            self.net.load_state_dict(ck["net_state_dict"])
        steps = load_adam_state_dict(self.net, self.optimizer, ck["optimizer_state_dict"], per_param=True)
        for (n, _), st in zip(self.net.named_parameters(), steps):
            self.optimizer.steps[self._group_of[n]] = st
        self.learn_step = int(ck["learn_step"])
        sn = ck.get("state_norm")
        if isinstance(sn, dict):
            self.state_norm.load_state_dict(sn)
        self.round_count = int(ck.get("round_count", self.round_count))   # Philox counter base and per-round env seed
        if isinstance(ck.get("reward_scaling"), dict):
            self.reward_scaler.load_state_dict(ck["reward_scaling"])
        print(f"Model loaded from {self.cfg.save_path}")

    # ------------------------------------------------------------------- train ---
    def _update_print(self, metrics):
        print(f"  Update - Loss: {metrics['total_loss']:.4f}, Aux: {metrics['aux_value_loss']:.4f}")

    def train(self):
        """:431-499 by rounds of num_envs episodes."""
        cfg = self.cfg
        print("Starting training...")
        episode, solved = 0, False
        while episode < cfg.max_episodes and not solved:
            returns, lengths = self.collect_round()
            for i in range(self.N):
                if episode >= cfg.max_episodes:
                    break
                self.episode_rewards.append(returns[i])
                avg = float(np.mean(self.episode_rewards))
                print(f"Episode {episode + 1}/{cfg.max_episodes} | Reward: {returns[i]:.0f} | Avg(100): {avg:.1f} | "
                      f"Steps: {lengths[i]}")
                if (episode + 1) % cfg.batch_size == 0 and episode > 0:
                    self._update_print(self.update())
                elif (episode + 1) % cfg.batch_size == 0:
                    # batch_size == 1: the `episode > 0` guard skips the update after episode 0.  The reference then
                    # appends episode 1 to the same buffer slot and trains on both as one sequence; here episode 0's
                    # data is dropped, so every update trains on whole episodes.
                    self._batch = []
                if (episode + 1) % cfg.save_freq == 0:
                    self.save_model()
                episode += 1
                if avg >= 200.0 and len(self.episode_rewards) >= 100:
                    print(f"\nEnvironment solved in {episode} episodes!")
                    solved = True
                    break
        print("Training completed!")
        self.save_model()
        self.env.close()

    EVAL_SEED_OFFSET, EVAL_ENV_ID0 = 1_000_003, 1 << 40      # eval()'s env streams: seed base_seed + 1_000_003, env ids from 1 << 40

    def _eval_fusable(self):
        """Whether gymrl_lunar_mlprnn_eval plays this trainer's env: the built-in LunarLander-v3 (8 observations, 4 actions)."""
        return ops.ENV_KINDS.get(self._env_name()) == ops.LUNARLANDER and self.state_dim == 8 and self.action_dim == 4

    @torch.no_grad()
    def evaluate(self, num_episodes, params=None, norm_stats=None, stream_offset=0):
        """-> (returns f64, lengths i32, terminated u8), numpy arrays [P, num_episodes]: whole greedy episodes on eval()'s streams
        (episode e: seed base_seed + 1_000_003, env id (1 << 40) + stream_offset + e), every policy from the same starts and from
        the hidden state 0, in ONE launch (csrc/eval_lunar_rnn.hip) whatever Config.fused_eval says.  params = None: the trainer's
        own policy (P = 1); params = f32[P, n]: a stack of flat parameter vectors in the layout of flat_params.  norm_stats = None:
        the trainer's state_norm statistics as they are now, for every policy; f64[26] or f64[P, 26]: RunningMeanStd.stats to
        normalise the observations with instead.  Actions, lengths and terminal observations are eval()'s loop's, bit for bit.
        Moves neither round_count, net.rnn_h, state_norm, reward_scaler, self.env, the batch nor the optimiser."""
        if not self._eval_fusable():
            raise RuntimeError("PPGTrainer.evaluate: gymrl_lunar_mlprnn_eval takes LunarLander-v3 (include/gymrl.h)")
        stats = self.state_norm.running_ms.stats if norm_stats is None else \
            torch.as_tensor(norm_stats, dtype=torch.float64).to(self.device).contiguous()
        policy = self._act_params
        if params is not None:
            params = torch.as_tensor(params, dtype=torch.float32).to(self.device)
            policy = ops.MlprnnPolicyStack(self.net, self.flat_params, params.view(1, -1) if params.dim() == 1 else params)
        out = ops.lunar_mlprnn_eval(policy, int(num_episodes), self.base_seed + self.EVAL_SEED_OFFSET,
                                    self.EVAL_ENV_ID0 + int(stream_offset), norm_stats=stats, want_terminal_obs=False)
        return tuple(t.cpu().numpy() for t in out[:3])

    def _eval_fused(self, n):
        """eval(n)'s returns as one launch, or None: fused_eval is off, or the env is not the built-in LunarLander-v3."""
        if not getattr(self.cfg, "fused_eval", False) or n < 1 or not self._eval_fusable():
            return None
        returns = ops.lunar_mlprnn_eval(self._act_params, n, self.base_seed + self.EVAL_SEED_OFFSET, self.EVAL_ENV_ID0,
                                        norm_stats=self.state_norm.running_ms.stats, want_terminal_obs=False)[0]
        return returns[0].to(torch.float32).tolist()           # the float32 cast of the float64 return

    @torch.no_grad()
    def eval(self, num_episodes=10):
        """:501-524 as `num_episodes` parallel greedy episodes (state_norm without update), each with its own GRU state.  With
        Config.fused_eval the same episodes are ONE launch (gymrl_lunar_mlprnn_eval): the same actions, lengths and terminal
        observations bit for bit; the loop below sums an episode's rewards in float32, the launch in float64, so a printed
        return may differ from the loop's in the last place."""
        print(f"\nEvaluating for {num_episodes} episodes...")
        rewards = self._eval_fused(int(num_episodes))
        if rewards is None:
            rewards = self._eval_loop(int(num_episodes))
        for ep, r in enumerate(rewards):
            print(f"  Episode {ep + 1}: Reward = {r:.0f}")
        print(f"Evaluation: Mean = {np.mean(rewards):.1f} +/- {np.std(rewards):.1f}")
        return rewards

    def _eval_loop(self, n):
        dev = self.device
        env = VecEnv(self._env_name(), n, device=dev, seed=self.base_seed + self.EVAL_SEED_OFFSET, env_id0=self.EVAL_ENV_ID0)
        raw, term = env.reset(), torch.empty(n, self.state_dim, device=dev)
        rew = torch.empty(n, device=dev)
        terminated, truncated = (torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(2))
        live = torch.ones(n, dtype=torch.uint8, device=dev)
        ret = torch.zeros(n, device=dev)
        hidden = torch.zeros(n, 64, device=dev)
        s = torch.empty(n, self.state_dim, device=dev)
        act = torch.zeros(n, dtype=torch.int32, device=dev)
        lp, val = torch.empty(n, device=dev), torch.empty(n, device=dev)
        ops.running_norm_masked(raw, live, self.state_norm.running_ms.stats, update=False, out=s)
        for t in range(env.max_steps + 1):
            ops.mlprnn_act(s, hidden, self._act_params, self.action_dim, live=live, deterministic=True, h_out=hidden,
                           act_out=act, logp_out=lp, value_out=val)
            env.step(act, raw, rew, term_obs_out=term, terminated_out=terminated, truncated_out=truncated)
            ret.add_(rew * live)
            live.mul_(1 - (terminated | truncated))
            ops.running_norm_masked(term, live, self.state_norm.running_ms.stats, update=False, out=s)
            if (t + 1) % 16 == 0 and not bool(live.any()):
                break
        env.close()
        return ret.cpu().tolist()

    def test(self):
        """:526-547 — load + eval(5); there is no renderer, so the human-render episode is not played."""
        self.load_model()
        return self.eval(num_episodes=5)


if __name__ == "__main__":       # python -m gymrl_amd.ppg_rnn_lunarlander [--<Config attribute> <value> ...]  (:550-566)
    from .utils.cli import run_script
    run_script(Config, PPGTrainer)

"""NoisyNet dueling DQN — MI355X engine behind the reference's algorithms/noisy_dqn_cartpole.py surface:
Config :33-46, NoisyLinear :49-99, NoisyDuelingQNetwork :102-137, ReplayBuffer :140-161, NoisyDQNTrainer :164-338
(select_action :198-212, update :214-257, train :259-300).

The train / eval / checkpoint plumbing, the device replay ring with its keyed index draw, FusedAdam and GradSink are
dqn_cartpole's; NoisyLinear is Rainbow's (same init, same f(x) = sign(x) sqrt|x|, same counter-keyed Philox draw) with
sigma_init passed through.  What differs from DQN, and is stated here:

  * no epsilon-greedy: acting is the argmax of the noisy Q (the first maximum wins, as torch.argmax);
  * the target is double-Q: a* = argmax policy_net(s'), y = r + gamma target_net(s')[a*] (1 - d);
  * the loss is plain F.mse_loss: dq = 2 (q - y) / B on the taken action, no importance weights, no gradient clamp;
  * the hard target copy happens when learn_step % target_update_freq == 0 (learn steps, not episodes);
  * with num_envs = N one noise draw serves all N rows of a forward, as NoisyLinear does for any batch.

The noise.  The reference's update() cannot run as written: policy_net(next_states) under no_grad draws new noise IN PLACE into
the tensors that policy_net(states) saved for the gradient of sigma, and loss.backward() raises.  The intended semantics are
kept here: the gradient flows through the draw of policy_net(states) (set A), the action choice on s' uses a second,
independent draw (set B), the target network is in eval() and uses mu only, acting draws a third set (set C) per forward,
deterministic=True uses mu only.  Every draw is keyed by (layer seed, counter) with counters handed out in the reference's
order — C at select_action, then A, then B at update() — so the ORDER OF EXECUTION is free: the layer path runs the two
no_grad forwards first (as the reference's older legacy script does) and policy_net(states) last, and nothing is overwritten
under autograd.

With Config.fused_step the vector step is csrc/noisy_dqn_step.hip: gymrl_ndqn_combine (the effective parameters of sets C, A,
B in one launch), gymrl_ndqn_act_step, gymrl_ndqn_update (rows, tiles, split + Adam); sixteen steps replay as one hipGraph.
The default is the layer-by-layer path: three forwards of four layers, a noise launch per layer and forward, the backward
through the autograd of mu + sigma * eps.  update() returns {"loss"} on both paths and adds "q_mean" on the layer path.
"""
import copy
import struct
from collections import deque

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .dqn_cartpole import DQNTrainer, ReplayBuffer  # noqa: F401  (ReplayBuffer: the reference's surface)
from .envs import EpisodeTracker, VecEnv
from .flat import FusedAdam, GradSink, flatten_module
from .nn import _FusedLinear, _act_torch, _fusable, small_linear
from .rainbow_dqn_cartpole import NoisyLinear as _NoisyLinear
from .utils import scalar


class Config:
    def __init__(self):
        self.env_name = "CartPole-v1"
        self.seed = None
        self.max_episodes = 500
        self.max_steps = 10000
        self.batch_size = 64
        self.gamma = 0.99
        self.lr = 0.001
        self.target_update_freq = 500        # learn steps
        self.memory_capacity = 10000
        self.hidden_dim = 64
        self.sigma_init = 0.5
        self.device = "cuda"
        # --- vectorised-engine additions (defaults keep the reference's per-step cadence) ---
        self.num_envs = 1
        self.updates_per_step = 1            # reference: one update() per env step (:273)
        self.use_graphs = True               # replay the update as one captured hipGraph (train(); update() stays eager)
        self.fused_step = False              # the vector step as csrc/noisy_dqn_step.hip's launches: opt-in
        self.chunk_steps = 16                # vector steps per captured hipGraph on the fused path
        self.fused_eval = False              # eval() as ONE launch of whole episodes (csrc/eval_duel.hip): opt-in, the same list


def _linear(x, weight, bias, act=None):
    """act(x W^T + b) as one csrc/lin.hip launch per direction on the GPU (a non-leaf weight hands its gradient to autograd)."""
    if _fusable(x, weight):
        return _FusedLinear.apply((1, False, (ops.LIN_ACT[act],), (0.0,), (0.0,)), x, weight, bias)[0]
    return _act_torch(small_linear(x, weight, bias), act, (0.0, 0.0))


class NoisyLinear(_NoisyLinear):
    """:49-99.  Rainbow's layer (state-dict keys weight_mu ... bias_epsilon, the epsilon buffers persistent) whose draw is
    keyed by a counter its owner sets: `draw` = ("counter", c) | ("dev", device u64[1]) | ("raw", (eps_in_raw, eps_out_raw))."""

    draw = ("counter", 0)

    def reset_noise(self):
        if not self.weight_epsilon.is_cuda:
            return                        # CPU construction time: the buffers are filled on the first GPU forward
        kind, v = self.draw
        kw = dict(seed=self.seed, counter=v) if kind == "counter" else dict(seed=self.seed, counter_dev=v) if kind == "dev" else {}
        raw = v if kind == "raw" else (None, None)
        ops.noisy_noise(self.in_features, self.out_features, self.weight_epsilon, self.bias_epsilon, raw[0], raw[1], **kw)

    def forward(self, x, act=None):
        if self.training:
            self.reset_noise()            # new noise on every training-mode forward (:90-91)
            weight = self.weight_mu + self.weight_sigma.mul(self.weight_epsilon)
            bias = self.bias_mu + self.bias_sigma.mul(self.bias_epsilon)
        else:
            weight, bias = self.weight_mu, self.bias_mu
        return _linear(x, weight, bias, act)


class NoisyDuelingQNetwork(nn.Module):
    """:102-137 (same module tree, so reference state_dicts load unchanged).  Layer l draws under seed 4 * seed + l."""

    LAYERS = ops.NDQN_LAYERS

    def __init__(self, state_dim, action_dim, hidden_dim=64, sigma_init=0.5, seed=0):
        super().__init__()
        self.fc1 = NoisyLinear(state_dim, hidden_dim, sigma_init, seed=4 * seed)
        self.fc2 = NoisyLinear(hidden_dim, hidden_dim, sigma_init, seed=4 * seed + 1)
        self.value_stream = NoisyLinear(hidden_dim, 1, sigma_init, seed=4 * seed + 2)
        self.advantage_stream = NoisyLinear(hidden_dim, action_dim, sigma_init, seed=4 * seed + 3)
        self._draws = 0

    def set_draw(self, kind, value):
        """The next training-mode forward's noise: ("counter", c), ("dev", u64[1] on the device) or ("raw", f32 row holding per
        layer the input-side N(0,1) draws, then the output-side ones)."""
        o = 0
        for name in self.LAYERS:
            m = getattr(self, name)
            if kind == "raw":
                i, n = m.in_features, m.out_features
                m.draw = ("raw", (value[o:o + i], value[o + i:o + i + n]))
                o += i + n
            else:
                m.draw = (kind, value)

    def forward(self, x):
        x = self.fc2(self.fc1(x, act="relu"), act="relu")
        value, advantage = self.value_stream(x), self.advantage_stream(x)
        return value + (advantage - advantage.mean(dim=-1, keepdim=True))

    def reset_noise(self):
        """:133-137 — a fresh draw into every layer's epsilon buffers (the module's own counter)."""
        self._draws += 1
        self.set_draw("counter", (1 << 40) + self._draws)
        for name in self.LAYERS:
            getattr(self, name).reset_noise()


class NoisyDQNTrainer(DQNTrainer):
    CHUNK_FIELDS = [("push", "q"), ("noise", "3Q"), ("draw", "Qq"), ("adam", "4f")]     # one step's device record

    def __init__(self, config):
        self.cfg = config
        if not torch.cuda.is_available() or not ops.device_ok():
            raise RuntimeError("gymrl_amd.NoisyDQNTrainer needs an MI355X and libgymrl_hip.so; no CPU fallback")
        self.device = torch.device(config.device if ":" in str(config.device) else f"cuda:{torch.cuda.current_device()}")
        self.base_seed = 0 if config.seed is None else int(config.seed)
        self.env = VecEnv(config.env_name, config.num_envs, device=self.device, seed=self.base_seed)
        state_dim, action_dim = self.env.observation_space.shape[0], self.env.action_space.n
        self.action_dim = action_dim
        g = torch.random.get_rng_state()
        torch.manual_seed(self.base_seed)
        self.policy_net = NoisyDuelingQNetwork(state_dim, action_dim, config.hidden_dim, config.sigma_init, seed=self.base_seed)
        torch.random.set_rng_state(g)
        self.target_net = copy.deepcopy(self.policy_net)
        self.flat_params, self.flat_grads = flatten_module(self.policy_net, self.device)
        self.target_flat, _ = flatten_module(self.target_net, self.device)
        self.target_net.eval()
        self._sink = GradSink(self.policy_net)
        self.optimizer = FusedAdam(self.flat_params, self.flat_grads, lr=config.lr, eps=1e-8)      # optim.Adam(lr): no clamp
        self.memory = self._make_memory(state_dim)
        self.learn_step = 0
        self.noise_draws = 0           # counters handed out so far: C at select_action, then A, B at update()
        self.epsilon, self.sample_count, self._act_counter = 0.0, 0, 0       # (DQN's checkpoint fields: unused here)
        self.episode_rewards = deque(maxlen=100)
        self._loss = torch.zeros(1, dtype=torch.float64, device=self.device)
        self._parity_indices = None    # tests: iterator of i32[B] replay indices for update()
        self._parity_raw_act = None    # tests: iterator of f32 raw rows for select_action's draw
        self._parity_raw = None        # tests: iterator of (raw row A, raw row B) for update()'s draws
        self._graph = None             # hipGraph of the layer-path update, captured on first use (update_async)
        self._chunks = {}              # fused path: target-copy pattern -> its captured StepChunk

    def _next_draw(self):
        self.noise_draws += 1
        return self.noise_draws

    def _eval_duel_policy(self):
        """eval() acts on mu only (select_action(deterministic=True)): every layer's weight_mu / bias_mu, no draw, and neither
        `noise_draws` nor policy_net.training moves (csrc/eval_duel.hip)."""
        net = self.policy_net
        pair = lambda m: (m.weight_mu, m.bias_mu)     # noqa: E731
        return [pair(net.fc1), pair(net.fc2)], pair(net.value_stream), pair(net.advantage_stream), self.flat_params

    # ------------------------------------------------------------ acting (:198-212) ---------------------------
    @torch.no_grad()
    def select_action(self, state, deterministic=False, raw=None):
        """[N, D] states -> i32[N] (device in, device out), or the reference's scalar surface: one np.ndarray [D] -> int.
        raw: a float32 raw row in place of the keyed draw (parity mode)."""
        state, kind = scalar.obs_batch(state, self.device)
        net = self.policy_net
        if deterministic:              # mu only, and the draw counter does not move (bit-exact resume / replay)
            net.eval()
            q = net(state)
            net.train()
        else:
            if raw is None and self._parity_raw_act is not None:
                raw = next(self._parity_raw_act)
            if raw is not None:
                net.set_draw("raw", raw)
            else:
                net.set_draw("counter", self._next_draw())
            q = net(state)
        self._last_q = q
        # epsilon 0: the greedy action of gymrl_epsilon_greedy — the first maximum, torch.argmax's rule
        return scalar.discrete_out(ops.epsilon_greedy(q, 0.0, seed=self.base_seed, counter=0, env_id0=self.env.env_id0), kind)

    def load_target(self):
        self.target_flat.copy_(self.flat_params)        # target_net.load_state_dict(policy_net.state_dict()): the parameters

    def _after_update(self):
        """:250-252."""
        self.learn_step += 1
        if self.learn_step % self.cfg.target_update_freq == 0:
            self.load_target()

    # ------------------------------------------------------------ update (:214-257) ---------------------------
    def update(self, indices=None, raw=None):
        """:214-257.  -> {} while the memory is short, else {"loss": float} (one host sync, like loss.item()), with "q_mean" on the
        layer path.  indices: explicit replay rows; raw = (row A, row B): raw draws in place of the keyed ones."""
        cfg = self.cfg
        if len(self.memory) < cfg.batch_size:
            return {}
        if indices is None and self._parity_indices is not None:
            indices = next(self._parity_indices)
        if raw is None and self._parity_raw is not None:
            raw = next(self._parity_raw)
        if self._fused_update_ok() and (indices is None or indices.numel() == cfg.batch_size):
            self._combine(raw=None if raw is None else (None, raw[0], raw[1]), act=False)
            self._update_fused(indices)
            self._after_update()
            return {"loss": float(self._loss.item()) / cfg.batch_size}
        if indices is None:
            indices = self.memory.draw_indices(cfg.batch_size)
        draws = (("raw", raw[0]), ("raw", raw[1])) if raw is not None else (("counter", self._next_draw()), ("counter", self._next_draw()))
        n = self._update_body(indices, draws)
        self._after_update()
        return {"loss": float(self._loss.item()) / n, "q_mean": float(self._q_taken.mean().item())}

    def _update_body(self, indices, draws, bias=None):
        """Everything after the index draw.  draws = (set A's, set B's) as set_draw arguments; bias = f32[4] device view of Adam's
        step scalars under a hipGraph.  The no_grad forwards run FIRST (see the module docstring)."""
        states, actions, rewards, next_states, dones = self.memory.gather(indices)
        net = self.policy_net
        with torch.no_grad():
            net.set_draw(*draws[1])
            qn_online = net(next_states)                                       # :238
            qn = self.target_net(next_states)                                  # :239 (eval(): mu only)
        net.set_draw(*draws[0])
        q = net(states)                                                        # :235
        self._loss.zero_()
        td, dq = ops.dqn_td_loss(q, qn, actions.view(-1), rewards, dones, self.cfg.gamma, q_next_online=qn_online,
                                 loss_sum=self._loss)                          # :236-243: F.mse_loss, dq = 2 td / B
        self._q_taken = q.detach().gather(1, actions.view(-1, 1).long()) if bias is None else None
        self._sink.arm()
        q.backward(dq)
        self._sink.collect()
        self.optimizer.step(bias_dev=bias)
        return states.shape[0]

    def update_async(self):
        """update() without the host round trip: eager index draw + one scalar store (Adam's bias and the two draw counters),
        then the captured hipGraph of `_update_body`.  The loss sum stays on the device; the target copy runs behind the replay."""
        cfg, m = self.cfg, self.memory
        if len(m) < cfg.batch_size:
            return
        if self._fused_update_ok():
            self._combine(act=False)
            self._update_fused()
            return self._after_update()
        if self._graph is None:
            from .graphs import GraphedStep, StepScalars
            self._scalars = StepScalars(self.device)
            bias, self._off = self._scalars.slot(16, torch.float32)
            (ca, self._off_a), (cb, self._off_b) = self._scalars.slot(8, torch.uint8), self._scalars.slot(8, torch.uint8)
            self._g_idx = torch.empty(cfg.batch_size, dtype=torch.int32, device=self.device)
            self._graph = GraphedStep(lambda: self._update_body(self._g_idx, (("dev", ca), ("dev", cb)), bias=bias))
        m.draw_indices(cfg.batch_size, out=self._g_idx)
        self._scalars.set(self._off, self.optimizer.next_bias())
        self._scalars.set(self._off_a, struct.pack("=Q", self._next_draw()))
        self._scalars.set(self._off_b, struct.pack("=Q", self._next_draw()))
        self._scalars.flush()
        self._graph()
        self._after_update()

    # ------------------------------------------------------------ fused vector step (csrc/noisy_dqn_step.hip) -
    def _fused_update_ok(self):
        cfg, m = self.cfg, self.memory
        return (bool(getattr(cfg, "fused_step", False)) and m.capacity < 1 << 30
                and ops.ndqn_fused_shape_ok(cfg.batch_size, m.ring[0].shape[1], self.action_dim, cfg.hidden_dim))

    def _fused_args(self):
        if self._fused is None or self._fused[3] is not self.env:
            cfg, env, m = self.cfg, self.env, self.memory
            D, A = m.ring[0].shape[1], self.action_dim
            ws = ops.ndqn_update_workspace(cfg.batch_size, D, A, cfg.hidden_dim, self.device)
            act = (ops.ndqn_act_args(env, self.policy_net, m.ring, m.capacity, ws)
                   if isinstance(env, VecEnv) and env.kind == ops.CARTPOLE else None)
            upd = ops.ndqn_update_args(cfg.batch_size, D, A, self.policy_net, self.target_net, self.optimizer, m.ring, cfg.gamma,
                                       self._loss, ws)
            comb = ops.ndqn_combine_args(D, A, self.policy_net, ws)
            self._fused = (act, upd, ws, env, comb)
        return self._fused

    def _combine(self, raw=None, act=True, update=True, dev=None):
        """The step's gymrl_ndqn_combine launch.  The counters are handed out in the layer path's order: C where the step acts,
        then A and B where it updates (an unused set is formed under counter 0 and read by nobody).  dev: device u64[3]."""
        comb = self._fused_args()[4]
        if dev is not None:
            return ops.ndqn_combine(comb, counter_dev=dev)
        raw = raw or (None, None, None)
        c = self._next_draw() if act and raw[0] is None else 0
        ab = (self._next_draw(), self._next_draw()) if update and raw[1] is None else (0, 0)
        ops.ndqn_combine(comb, counters=(c, *ab), raw=raw)

    def _update_fused(self, indices=None, dev=None):
        """gymrl_ndqn_update's three launches behind this step's combine.  dev = (draw, adam) device records of a StepChunk
        replay; None: this call's scalars travel as arguments and the host counters advance here."""
        m = self.memory
        upd = self._fused_args()[1]
        if dev is not None:
            return ops.ndqn_update(upd, idx_seed=m.seed, idx_dev=dev[0], idx_size=m.capacity, adam_policy_dev=dev[1])
        if indices is None:
            counter, size = m.draws, m.size
            m.draws += 1
        else:
            counter, size = 0, 0
            if indices.dtype != torch.int32:
                indices = indices.to(torch.int32)
        ops.ndqn_update(upd, idx=indices, idx_seed=m.seed, idx_counter=counter, idx_size=size, adam_policy=self.optimizer.next_bias())

    def _act_fused(self, lb, obs, nxt, ep_ret, done, dev=None):
        """Acting + env step + replay row of one vector step on set C: one launch.  dev: the push cursor's device record."""
        env, m = self.env, self.memory
        ops.ndqn_act_step(self._fused_args()[0], env, obs, nxt, cursor=m.cursor, cursor_dev=dev, rew_out=lb["rew"], done_out=done,
                          ep_ret_out=ep_ret, ep_stats=env.ep_stats)
        if dev is None:
            m.advance(env.n)

    def _explicit_draws(self):
        """Whether a test feeds raw draws of its own: a StepChunk replay reads only the kernels' Philox keys."""
        return self._parity_raw is not None or self._parity_raw_act is not None

    def _copy_pattern(self, K):
        """The steps of the next K updates behind which the hard target copy falls."""
        f = self.cfg.target_update_freq
        return tuple(j for j in range(K) if (self.learn_step + j + 1) % f == 0)

    def _chunk_body(self, lb, j, pattern):
        ch, tr = self._chunk, lb["tracker"]
        obs, nxt = (lb["obs"], lb["nxt"]) if j % 2 == 0 else (lb["nxt"], lb["obs"])
        self._combine(dev=ch.view(j, "noise"))
        self._act_fused(lb, obs, nxt, tr.ret[j], tr.done[j], dev=ch.view(j, "push"))
        self._update_fused(dev=(ch.view(j, "draw"), ch.view(j, "adam", torch.float32)))
        if j in pattern:
            self.load_target()         # a device copy of the flat parameters: a node of the graph

    def _stage_chunk(self):
        """The host's bookkeeping of the next K vector steps, in the eager loop's order, written into the records."""
        ch, m, N = self._chunk, self.memory, self.env.n
        for j in range(ch.K):
            ch.set(j, "push", m.cursor)
            m.advance(N)
            ch.set(j, "noise", self._next_draw(), self._next_draw(), self._next_draw())
            self._stage_draw(j)
            ch.set_bytes(j, "adam", self.optimizer.next_bias())
            self.learn_step += 1
        ch.flush()

    def _train_fused(self, max_vector_steps=None):
        """_train on the fused step: combine, act, rows, tiles, split + Adam per vector step (+ the copy when due).  With
        hipGraphs on, chunk_steps whole vector steps replay as one graph (graphs.StepChunk), one captured graph per pattern of
        target copies inside the chunk; while the ring holds fewer rows than a batch, and for what a chunk cannot take, the
        loop is eager."""
        cfg, env, m = self.cfg, self.env, self.memory
        N, D, K = env.n, env.obs_dim, int(cfg.chunk_steps)
        self.CHUNK = K
        lb = self._loop_buffers(N, D)
        obs, nxt, tracker = lb["obs"], lb["nxt"], lb["tracker"]
        env.reset(obs)
        step = 0
        graphed = bool(getattr(cfg, "use_graphs", True)) and self._parity_indices is None
        chunked = graphed and N > 1 and not self._explicit_draws() and K % 2 == 0
        limit = max_vector_steps or (cfg.max_episodes * cfg.max_steps // N + 1)
        solved = lambda: len(self.episode_rewards) >= 100 and np.mean(self.episode_rewards) >= 495.0   # noqa: E731
        while tracker.episodes < cfg.max_episodes and step < limit:
            if (chunked and tracker.k == 0 and limit - step >= K and obs is lb["obs"] and len(m) >= cfg.batch_size and not solved()):
                pattern = self._copy_pattern(K)
                ch = self._chunks.get(pattern)
                if ch is None:
                    from .graphs import StepChunk
                    ch = self._chunks[pattern] = StepChunk(self.device, K, self.CHUNK_FIELDS)
                self._chunk = ch
                self._fused_args()
                self._stage_chunk()
                ch.run(lambda j: self._chunk_body(lb, j, pattern), key=(id(env), env.state.data_ptr()))
                step += K
                tracker.k = K
                tracker.flush(self.episode_rewards)
            else:
                ep_ret, done = tracker.slot()
                will_update = min(m.size + N, m.capacity) >= cfg.batch_size
                raw_c = None if self._parity_raw_act is None else next(self._parity_raw_act)
                raw_ab = (None, None) if self._parity_raw is None or not will_update else next(self._parity_raw)
                self._combine(raw=(raw_c, *raw_ab), update=will_update)
                self._act_fused(lb, obs, nxt, ep_ret, done)
                if will_update:
                    self._update_fused(None if self._parity_indices is None else next(self._parity_indices))
                    self._after_update()
                obs, nxt = nxt, obs
                step += 1
                tracker.advance(self.episode_rewards)
            if solved():
                break
        tracker.flush(self.episode_rewards)
        self.env.close()

    def _loop_buffers(self, N, D):
        lb = getattr(self, "_loop", None)
        if lb is None or lb["N"] != N or lb["tracker"].K != (1 if N == 1 else self.CHUNK):
            self._loop = None
        return super()._loop_buffers(N, D)

    # ------------------------------------------------------------ train (:259-300) ----------------------------
    def _train(self, max_vector_steps=None):
        """:259-300 with N lock-stepped envs; "episodes" counts finished episodes over all envs."""
        cfg, env = self.cfg, self.env
        if self._fused_ok():
            return self._train_fused(max_vector_steps)
        N, D = env.n, env.obs_dim
        obs, nxt, tobs = (torch.empty(N, D, device=self.device) for _ in range(3))
        rew = torch.empty(N, device=self.device)
        tracker = EpisodeTracker(N, self.device, flush_every=1 if N == 1 else 16)
        env.reset(obs)
        step = 0
        graphed = bool(getattr(cfg, "use_graphs", True)) and self._parity_indices is None and self._parity_raw is None
        limit = max_vector_steps or (cfg.max_episodes * cfg.max_steps // N + 1)
        while tracker.episodes < cfg.max_episodes and step < limit:
            action = self.select_action(obs)
            ep_ret, done = tracker.slot()
            env.step(action, nxt, rew, done_out=done, term_obs_out=tobs, ep_ret_out=ep_ret)
            self.memory.push(obs, action, rew, tobs, done)      # next_state = pre-reset observation (:272)
            if cfg.max_steps < env.max_steps:
                env.abandon(cfg.max_steps, nxt, done, ep_ret)
            for _ in range(cfg.updates_per_step):
                if graphed:
                    self.update_async()
                else:
                    self.update()
            obs, nxt = nxt, obs
            step += 1
            tracker.advance(self.episode_rewards)
            if len(self.episode_rewards) >= 100 and np.mean(self.episode_rewards) >= 495.0:
                break
        tracker.flush(self.episode_rewards)
        self.env.close()

    # ------------------------------------------------------------ checkpoint ----------------------------------
    def save_checkpoint(self, path, include_memory=True):
        from .utils import checkpoint
        extra = {"memory_state_dict": self.memory.state_dict()} if include_memory else {}
        return checkpoint.save_agent(path, {"policy_net": self.policy_net, "target_net": self.target_net},
                                     {"optimizer": (self.policy_net, self.optimizer)}, learn_step=self.learn_step,
                                     noise_draws=self.noise_draws, episode_rewards=list(self.episode_rewards), **extra)

    def load_checkpoint(self, path):
        from .utils import checkpoint
        rest = checkpoint.load_agent(path, {"policy_net": self.policy_net, "target_net": self.target_net},
                                     {"optimizer": (self.policy_net, self.optimizer)})
        self.learn_step, self.noise_draws = int(rest["learn_step"]), int(rest["noise_draws"])
        self.episode_rewards.clear()
        self.episode_rewards.extend(rest.get("episode_rewards", []))
        if "memory_state_dict" in rest:
            self.memory.load_state_dict(rest["memory_state_dict"])
        return rest


if __name__ == "__main__":       # python -m gymrl_amd.noisy_dqn_cartpole [--<Config attribute> <value> ...]  (:341-357)
    from .utils.cli import run_script
    run_script(Config, NoisyDQNTrainer)

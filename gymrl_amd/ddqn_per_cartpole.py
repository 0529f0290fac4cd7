"""Double DQN + prioritised replay — MI355X engine behind the reference's algorithms/ddqn_per_cartpole.py surface:
Config :31-51, QNetwork :54-64, SumTree :67-106, PrioritizedReplayBuffer :109-150, DDQNPERTrainer :153-329
(get_epsilon :179-184, select_action :186-195, update :197-244, train :246-288).

The train loop, acting, eval and the checkpoint are dqn_cartpole.DQNTrainer's (the two scripts' loops are the same text); what
this module states is what differs: nn.Linear's default init under the names fc1 / fc2 / fc3, the sum tree of PER "variant B"
(csrc/per.hip: `v <= left` descent, tree indices out, float64 weights, min(|td| + eps, error_max)^alpha) next to the replay
ring, the double-Q target with importance weights (gymrl_dqn_td_loss with q_next_online and w), and the TD errors going back
into the tree inside update().  ddqn_per_duel_cartpole.py imports everything here and replaces the network.

With Config.fused_step the update's forward chains, TD target and input-gradient chain are gymrl_ddqn_update's row launch
(csrc/ddqn_step.hip) and acting is gymrl_dqn_act_step (the dueling net: gymrl_ddqn_duel_act_step); the default is the
layer-by-layer path.  On MountainCar-v0 and Acrobot-v1 (`env_name`) the non-dueling trainer acts through
gymrl_dqn_act_step_classic (ops.FUSED_ACT_KINDS); the dueling one, whose kernels are two-action ones, trains layer by layer there.
"""
import numpy as np
import torch
import torch.nn as nn

from . import ops
from .dqn_cartpole import DQNTrainer, ReplayBuffer
from .envs import VecEnv
from .nn import SmallLinear
from .rainbow_dqn_cartpole import SumTree as _DeviceSumTree


class Config:
    def __init__(self):
        self.env_name = "CartPole-v1"
        self.seed = None
        self.max_episodes = 500
        self.max_steps = 10000
        self.batch_size = 64
        self.gamma = 0.9
        self.lr = 0.001
        self.epsilon_start = 0.95
        self.epsilon_end = 0.01
        self.epsilon_decay = 800
        self.target_update_freq = 4          # episodes
        self.memory_capacity = 65536
        self.hidden_dim = 256
        self.alpha = 0.6
        self.beta = 0.4                      # advanced by beta_increment in every sample() (:125), as in the reference
        self.beta_increment = 0.001
        self.error_max = 1.0
        self.eps = 1e-4
        self.device = "cuda"
        # --- vectorised-engine additions (defaults keep the reference's per-step cadence) ---
        self.num_envs = 1
        self.updates_per_step = 1            # reference: one update() per env step (:260)
        self.use_graphs = True               # replay the update as one captured hipGraph (train(); update() stays eager)
        self.fused_step = False              # the vector step as gymrl_dqn_act_step + gymrl_ddqn_update (csrc/ddqn_step.hip): opt-in
        self.fused_images = True             # ... with weight images of the H x H layer (H % 16 == 0)
        self.fused_eval = False              # eval() as ONE launch of whole episodes (csrc/eval_classic.hip): opt-in, the same list


class QNetwork(nn.Module):
    """ddqn_per_cartpole.py:54-64 (same module tree and nn.Linear's default init, so reference state_dicts load unchanged)."""

    def __init__(self, state_dim, action_dim, hidden_dim=256):
        super().__init__()
        self.fc1 = SmallLinear(state_dim, hidden_dim, act="relu")       # the ReLUs run inside the layers' launches (csrc/lin.hip)
        self.fc2 = SmallLinear(hidden_dim, hidden_dim, act="relu")
        self.fc3 = SmallLinear(hidden_dim, action_dim)

    def forward(self, x):
        return self.fc3(self.fc2(self.fc1(x)))


class SumTree(_DeviceSumTree):
    """:67-106 on a device float64 array (`tree`, 2 * capacity - 1 nodes, leaves last): Rainbow's device tree with the error
    clip of :144 in update_td.  `size` and `data_pointer` are the ring's and live in PrioritizedReplayBuffer."""

    def update_td(self, idx, td, alpha, eps, clip=0.0):
        """update_priorities (:142-147) of the data rows idx straight from the TD errors: min(|td| + eps, clip)^alpha in the
        leaf pass, the leaves' new maximum out of the same launches.  False: outside that kernel's range."""
        if idx.numel() > ops.PER_TD_MAX_BATCH or self.capacity >= 1 << 30:
            return False
        ops.per_update_td(self.tree, self.capacity, idx, td, alpha, eps, self._ws, clip=clip, max_out=self._max, ticket=self._ticket)
        self._max_fresh = True
        return True

    def store_at_max(self, start, n, empty, start_dev=None):
        """push (:114-117) for n consecutive rows: max(leaves), or 1.0 while that maximum is 0.  Priorities are
        min(.) ^ alpha of something >= eps > 0, so the maximum is 0 exactly while nothing was ever stored (`empty`).
        Writing the maximum itself leaves the maximum what it was: `_max` stays fresh."""
        if empty:
            self.update_range(start, n, priority=1.0)
            return
        mx = self.priority_max
        ops.per_update(self.tree, self.capacity, n, self._ws, idx_start=start, prio_scalar_dev=mx, idx_start_dev=start_dev)
        self._max_fresh = True

    def total_priority(self):
        return self.tree[0]


class PrioritizedReplayBuffer(ReplayBuffer):
    """:109-150 for N rows per push: dqn_cartpole's device ring with the sum tree beside it.  `indices` handed out by sample()
    and taken by update_priorities() are TREE indices (leaf = row + capacity - 1), as in the reference."""

    def __init__(self, config, state_dim=4, device=None, seed=0):
        if not config.eps > 0:
            raise ValueError("PrioritizedReplayBuffer needs eps > 0 (a stored priority is never 0)")
        super().__init__(config.memory_capacity, state_dim, torch.device(device or config.device), seed=seed)
        self.cfg = config
        self.tree = SumTree(self.capacity, self.device)
        self._draws = {}               # batch size -> fixed (tree index, priority, weight, ring row) buffers: captured graphs hold them

    def push(self, state, action=None, reward=None, next_state=None, done=None, cursor_dev=None):
        """:114-117.  push((state, action, reward, next_state, done)) as in the reference, or the five as arguments."""
        if action is None:
            state, action, reward, next_state, done = state
        cursor, empty = self.cursor, self.size == 0
        super().push(state, action, reward, next_state, done, cursor_dev=cursor_dev)
        n = int(reward.numel()) if torch.is_tensor(reward) else int(np.size(reward))
        self.store_priorities(cursor, n, empty, cursor_dev)

    def store_priorities(self, cursor, n, empty, cursor_dev=None):
        """The tree's half of push() for the n rows at `cursor` (the fused act launch writes the ring rows itself)."""
        if n > self.capacity:
            raise ValueError("memory_capacity must be >= the rows of one push")
        self.tree.store_at_max(cursor, n, empty, start_dev=cursor_dev)

    def next_beta(self):
        """:125 — host float64, before the draw."""
        self.cfg.beta = min(1.0, self.cfg.beta + self.cfg.beta_increment)
        return self.cfg.beta

    def draw(self, batch_size, u=None, dev=None):
        """The stratified draw of :119-138 -> (ring rows i32[B], is_weight f32[B], tree indices i32[B]), fixed buffers.
        u: f64[B] uniforms in place of the kernel's Philox; dev (StepChunk capture): device record {counter, size, beta}."""
        out = self._draws.get(batch_size)
        if out is None:
            d = self.device
            out = self._draws[batch_size] = (torch.empty(batch_size, dtype=torch.int32, device=d),
                                             torch.empty(batch_size, dtype=torch.float64, device=d),
                                             torch.empty(batch_size, dtype=torch.float32, device=d),
                                             torch.empty(batch_size, dtype=torch.int32, device=d))
        t = self.tree
        if dev is not None:
            ops.per_sample(t.tree, self.capacity, batch_size, 1, 0.0, t._ws, seed=self.seed, variant_b=True, out=out[:3], dev=dev)
        else:
            beta = self.next_beta()
            ops.per_sample(t.tree, self.capacity, batch_size, self.size, beta, t._ws, u=u, seed=self.seed, counter=self.draws,
                           variant_b=True, out=out[:3])
            self.draws += 1
        torch.sub(out[0], self.capacity - 1, out=out[3])        # leaf -> ring row: what the gather and the tree update take
        return out[3], out[2], out[0]

    def sample(self, batch_size, u=None):
        """:119-140 -> ((states, actions, rewards, next_states, dones), tree indices i32[B], is_weight f32[B])."""
        rows, w, leaves = self.draw(batch_size, u=u)
        return self.gather(rows), leaves.clone(), w.clone()

    def update_rows(self, rows, td):
        """update_priorities by ring row, from the TD errors themselves (device tensors; the sign is dropped in the kernel)."""
        cfg = self.cfg
        if td.dtype == torch.float32 and rows.dtype == torch.int32 and self.tree.update_td(rows, td, cfg.alpha, cfg.eps, cfg.error_max):
            return
        self.tree.update_batch(rows, ops.per_priorities(td, cfg.alpha, cfg.eps, clip=cfg.error_max))

    def update_priorities(self, indices, errors):
        """:142-147 — tree indices and |td| (tensors or numpy arrays), applied in batch order (last writer wins)."""
        d = self.device
        rows = torch.as_tensor(indices, device=d).to(torch.int32) - (self.capacity - 1)
        self.update_rows(rows.contiguous(), torch.as_tensor(errors, device=d).to(torch.float32).contiguous())

    def state_dict(self):
        """The ring and its cursors, the float64 tree, beta and the draw counter."""
        return {**super().state_dict(), "tree": self.tree.tree.detach().cpu(), "beta": float(self.cfg.beta)}

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        self.tree.tree.copy_(sd["tree"].to(self.device))
        # the device maximum is recomputed HERE: a StepChunk graph captured while it was fresh holds no launch that would
        ops.per_max_leaf(self.tree.tree, self.capacity, self.tree._max, self.tree._ws)
        self.tree._max_fresh = True
        self.cfg.beta = float(sd["beta"])


class DDQNPERTrainer(DQNTrainer):
    CHUNK_FIELDS = [("push", "q"), ("act", "Q"), ("eps", "f"), ("draw", "Qqd"), ("adam", "4f")]     # draw: gymrl_per_sample's record

    def __init__(self, config):
        super().__init__(config)
        B = config.batch_size
        self._parity_v = None          # tests: iterator of f64[B] stratified uniforms for sample()
        self._td = torch.zeros(B, device=self.device)          # the fused row launch's TD errors, on their way to the tree
        self._ones = torch.ones(B, device=self.device)         # is_weight of an explicit index list (_parity_indices)

    def _make_network(self, state_dim, action_dim, hidden_dim):
        return QNetwork(state_dim, action_dim, hidden_dim)

    def _make_memory(self, state_dim):
        return PrioritizedReplayBuffer(self.cfg, state_dim, self.device, seed=self.base_seed)

    # ------------------------------------------------------------ update (:197-244) ---------------------------
    def _draw(self, indices=None, dev=None):
        """-> (ring rows i32[B], is_weight f32[B]) of this update: the stratified draw, or an explicit row list with unit
        weights (beta does not move then)."""
        if indices is not None:
            # (a test hook, so one host round trip is fine: the ring AND the tree are indexed by these rows)
            if indices.numel() and not (0 <= int(indices.min()) and int(indices.max()) < self.memory.capacity):
                raise ValueError(f"update(): replay rows outside [0, {self.memory.capacity})")
            return (indices if indices.dtype == torch.int32 else indices.to(torch.int32)), self._ones[:indices.numel()]
        u = None if self._parity_v is None or dev is not None else next(self._parity_v)
        return self.memory.draw(self.cfg.batch_size, u=u, dev=dev)[:2]

    def update(self, indices=None):
        """:197-244.  Returns mean(td^2 * w) as a python float (one host sync, like loss.item())."""
        cfg = self.cfg
        if len(self.memory) < cfg.batch_size:
            return 0.0
        if indices is None and self._parity_indices is not None:
            indices = next(self._parity_indices)
        if self._fused_update_ok() and (indices is None or indices.numel() == cfg.batch_size):
            self._update_fused(indices)
            return float(self._loss.item()) / cfg.batch_size
        rows, w = self._draw(indices)
        n = self._update_body(rows, w)
        return float(self._loss.item()) / n

    def _update_body(self, rows, w, bias=None):
        """Everything after the draw, in the reference's order; bias = f32[4] device view of Adam's step scalars under a hipGraph."""
        self._images_stale()
        m = self.memory
        states, actions, rewards, next_states, dones = m.gather(rows)
        q = self.policy_net(states)                                            # :222
        with torch.no_grad():
            qn_online = self.policy_net(next_states)                           # :225
            qn = self.target_net(next_states)                                  # :226-228
        self._loss.zero_()
        td, dq = ops.dqn_td_loss(q, qn, actions.view(-1), rewards, dones, self.cfg.gamma, q_next_online=qn_online, w=w,
                                 loss_sum=self._loss)                          # :229-232
        self._last_td = td                                                     # (kept: the errors the tree has just taken)
        m.update_rows(rows, td)                                                # :234-235
        self._sink.arm()
        q.backward(dq)
        self._sink.collect()
        self.optimizer.step(bias_dev=bias)                                     # clamp +-1 (:239-241) inside the Adam kernel
        return states.shape[0]

    def update_async(self):
        """update() without the host round trip: the draw and one scalar store run eagerly, then the captured hipGraph of
        `_update_body`.  The loss sum stays on the device (`_loss`)."""
        cfg, m = self.cfg, self.memory
        if len(m) < cfg.batch_size:
            return
        if self._fused_update_ok():
            return self._update_fused()
        self._images_stale()
        if self._graph is None:
            from .graphs import GraphedStep, StepScalars
            self._scalars = StepScalars(self.device)
            bias, self._off = self._scalars.slot(16, torch.float32)
            self._graph = GraphedStep(lambda: self._update_body(*self._g_draw, bias=bias))
        self._g_draw = self._draw()                  # (the buffer's fixed tensors: the same two at every call)
        self._scalars.set(self._off, self.optimizer.next_bias())
        self._scalars.flush()
        self._graph()

    # ------------------------------------------------------------ fused vector step (csrc/ddqn_step.hip) ------
    DUELING = False                    # which instance of csrc/ddqn_step.hip's kernels the network is

    @staticmethod
    def _layers(net):
        """The network's three Linear layers in gymrl_ddqn_update_args' slots."""
        return net.fc1, net.fc2, net.fc3

    def _fused_update_ok(self):
        cfg, m = self.cfg, self.memory
        return (bool(getattr(cfg, "fused_step", False)) and m.capacity < 1 << 30
                and ops.ddqn_fused_shape_ok(cfg.batch_size, m.ring[0].shape[1], self.action_dim, cfg.hidden_dim, self.DUELING))

    def _fused_args(self):
        if self._fused is None or self._fused[3] is not self.env:
            cfg, env, m = self.cfg, self.env, self.memory
            D, A = m.ring[0].shape[1], self.action_dim
            img = (ops.dqn_images(cfg.hidden_dim, self.device)              # (the dueling net has no H x H layer: no images)
                   if getattr(cfg, "fused_images", True) and not self.DUELING else None)
            act = (ops.ddqn_act_args(env, self._layers(self.policy_net), m.ring, m.capacity, img)
                   if isinstance(env, VecEnv) and env.kind in ops.FUSED_ACT_KINDS       # (the dueling act kernel: two actions,
                   and (not self.DUELING or env.kind == ops.CARTPOLE) else None)        # and so CartPole only)
            ws = ops.ddqn_update_workspace(cfg.batch_size, D, A, cfg.hidden_dim, self.device)
            upd = ops.ddqn_update_args(cfg.batch_size, D, A, self._layers(self.policy_net), self._layers(self.target_net),
                                       self.optimizer, m.ring, cfg.gamma, self._td, self._loss, ws, img, dueling=self.DUELING)
            self._fused = (act, upd, ws, env, img)
            self._images_stale()
        if self._fused[4] is not None:
            self._refresh_images(((self.flat_params, self.policy_net), (self.target_flat, self.target_net)),
                                 ops.ddqn_pack_images, self._fused[1])
        return self._fused

    def _update_fused(self, indices=None, dev=None):
        """update() as the draw, gymrl_ddqn_update's two launches and the tree update.  dev = (draw, adam) device records of a
        StepChunk replay; None: this call's scalars travel as arguments and the host counters advance here."""
        upd = self._fused_args()[1]
        if dev is not None:
            rows, w = self._draw(dev=dev[0])
            ops.ddqn_update(upd, rows, w, adam_policy_dev=dev[1])
        else:
            rows, w = self._draw(indices)
            ops.ddqn_update(upd, rows, w, adam_policy=self.optimizer.next_bias())
        self._last_td = self._td
        self.memory.update_rows(rows, self._td)

    def _act_fused(self, lb, obs, nxt, ep_ret, done, dev=None):
        """DQN's act launch, then the N new rows enter the tree at the device-resident maximum."""
        m = self.memory
        cursor, empty = m.cursor, m.size == 0
        super()._act_fused(lb, obs, nxt, ep_ret, done, dev=dev)
        m.store_priorities(cursor, self.env.n, empty and dev is None, cursor_dev=None if dev is None else dev[0])

    def _explicit_draws(self):
        return self._parity_u is not None or self._parity_v is not None

    def _stage_draw(self, j):
        m = self.memory
        beta = m.next_beta()
        self._chunk.set(j, "draw", m.draws, m.size, beta)
        m.draws += 1


if __name__ == "__main__":       # python -m gymrl_amd.ddqn_per_cartpole [--<Config attribute> <value> ...]  (:332-348)
    from .utils.cli import run_script
    run_script(Config, DDQNPERTrainer)

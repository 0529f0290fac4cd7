"""Discrete SAC (expectation over actions, twin critics with separate optimisers, float32 temperature) —
MI355X engine behind the reference's algorithms/sac_cartpole.py surface: Config :28-43, ReplayBuffer :46-67,
Actor :70-80 (softmax output), Critic :83-93 (Q per action), SACTrainer :96-329 (select_action :127-138,
soft_update :140-145, update :148-227, train / eval / test).

With Config.fused_step the vector step is gymrl_dsac_act_step + gymrl_dsac_update (csrc/dsac_step.hip: one launch to act,
four to update, sixteen steps replayed as one hipGraph); the default is the layer-by-layer path described next.  On
MountainCar-v0 and Acrobot-v1 (`env_name`) the act launch is gymrl_dsac_act_step_classic (ops.FUSED_ACT_KINDS).

Underneath: CartPole instances step on the GPU; replay ring, categorical draw, soft-Bellman target, both
critic losses, the actor loss's forward + dL/dprobs, the float32 log_alpha Adam step, three fused Adam steps
and the Polyak updates are HIP kernels behind the C-ABI; Linear layers and the softmax run through PyTorch-ROCm.
"""
import copy
from collections import deque

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .dqn_cartpole import ReplayBuffer
from .envs import EpisodeTracker, VecEnv
from .flat import FusedAdam, GradSink, WeightImages, flatten_module
from .nn import SmallLinear
from .policy_eval import PolicyEval
from .utils import scalar


class Config:
    def __init__(self):
        self.env_name = "CartPole-v1"
        self.seed = None
        self.max_episodes = 500
        self.max_steps = 2000
        self.batch_size = 128
        self.gamma = 0.9
        self.tau = 0.005
        self.lr_actor = 2e-4
        self.lr_critic = 1e-3
        self.lr_alpha = 1e-3
        self.memory_capacity = 10000
        self.hidden_dim = 256
        self.target_entropy = -1.0
        self.device = "cuda"
        # --- vectorised-engine additions ---
        self.num_envs = 1
        self.updates_per_step = 1
        self.use_graphs = True             # replay the update as one captured hipGraph (train(); update() stays eager)
        self.fused_step = False            # the vector step as gymrl_dsac_act_step + gymrl_dsac_update (csrc/dsac_step.hip): opt-in
        self.fused_images = True           # ... with weight images of the H x H layers (H % 16 == 0)
        self.fused_eval = False            # eval() as ONE launch of whole episodes (csrc/eval_classic.hip): opt-in, the same list
        self.kernel_softmax = False        # Actor.forward through ops.softmax_rows (csrc/softmax_device.hpp) instead of F.softmax;
                                           # fused_step implies it (read when the trainer is built), so that the layer path and
                                           # the fused path of one run produce the same bits and the run can change paths


class Actor(nn.Module):
    def __init__(self, state_dim, action_dim, hidden_dim=256):
        super().__init__()
        self.fc1 = SmallLinear(state_dim, hidden_dim, act="relu")
        self.fc2 = SmallLinear(hidden_dim, hidden_dim, act="relu")
        self.fc3 = SmallLinear(hidden_dim, action_dim)
        self.kernel_softmax = False        # SACTrainer sets it from its Config

    def logits(self, x):
        return self.fc3(self.fc2(self.fc1(x)))

    def forward(self, x):
        z = self.logits(x)
        return ops.softmax_rows(z) if self.kernel_softmax else F.softmax(z, dim=-1)


class Critic(nn.Module):
    def __init__(self, state_dim, action_dim, hidden_dim=256):
        super().__init__()
        self.fc1 = SmallLinear(state_dim, hidden_dim, act="relu")
        self.fc2 = SmallLinear(hidden_dim, hidden_dim, act="relu")
        self.fc3 = SmallLinear(hidden_dim, action_dim)

    def forward(self, x):
        return self.fc3(self.fc2(self.fc1(x)))


class SACTrainer(WeightImages, PolicyEval):
    def __init__(self, config):
        self.cfg = config
        if not torch.cuda.is_available() or not ops.device_ok():
            raise RuntimeError("gymrl_amd.sac_cartpole.SACTrainer needs an MI355X and libgymrl_hip.so; no CPU fallback")
        self.device = torch.device(config.device if ":" in str(config.device) else f"cuda:{torch.cuda.current_device()}")
        self.base_seed = 0 if config.seed is None else int(config.seed)
        self.env = VecEnv(config.env_name, config.num_envs, device=self.device, seed=self.base_seed)
        state_dim, action_dim = self.env.observation_space.shape[0], self.env.action_space.n
        self.action_dim = action_dim
        g = torch.random.get_rng_state()
        torch.manual_seed(self.base_seed)
        self.actor = Actor(state_dim, action_dim, config.hidden_dim)
        self.actor.kernel_softmax = bool(getattr(config, "kernel_softmax", False) or getattr(config, "fused_step", False))
        self.critic1 = Critic(state_dim, action_dim, config.hidden_dim)
        self.critic2 = Critic(state_dim, action_dim, config.hidden_dim)
        torch.random.set_rng_state(g)
        self.critic1_target, self.critic2_target = copy.deepcopy(self.critic1), copy.deepcopy(self.critic2)
        self.actor_flat, self.actor_grads = flatten_module(self.actor, self.device)
        self.c1_flat, self.c1_grads = flatten_module(self.critic1, self.device)
        self.c2_flat, self.c2_grads = flatten_module(self.critic2, self.device)
        self.c1_target_flat, _ = flatten_module(self.critic1_target, self.device)
        self.c2_target_flat, _ = flatten_module(self.critic2_target, self.device)
        self._actor_sink, self._c1_sink, self._c2_sink = GradSink(self.actor), GradSink(self.critic1), GradSink(self.critic2)
        self.actor_optim = FusedAdam(self.actor_flat, self.actor_grads, lr=config.lr_actor)
        self.critic1_optim = FusedAdam(self.c1_flat, self.c1_grads, lr=config.lr_critic)
        self.critic2_optim = FusedAdam(self.c2_flat, self.c2_grads, lr=config.lr_critic)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.log_alpha = torch.tensor([np.log(0.01)], **f32)                  # float32 scalar (:118-120)
        self._alpha_m, self._alpha_v = torch.zeros(1, **f32), torch.zeros(1, **f32)
        self._alpha_steps = 0
        d64 = dict(dtype=torch.float64, device=self.device)
        self._sums = torch.zeros(4, **d64)           # critic1, critic2 loss sums | actor loss sum, entropy sum: one buffer, so that
        self._sums_c, self._sums_a = self._sums[0:2], self._sums[2:4]    # the fused update writes what the loss kernels write
        self._alpha_loss = torch.zeros(1, **d64)
        self.memory = ReplayBuffer(config.memory_capacity, state_dim, self.device, seed=self.base_seed)
        self.episode_rewards = deque(maxlen=100)
        self._act_counter = 0
        self._parity_noise = None      # tests: iterator of f32[N, A] Exp(1) draws for select_action
        self._parity_indices = None    # tests: iterator of i32[B] replay indices for update()
        self._graph = None             # hipGraph of the update, captured on first use (update_async)

    @torch.no_grad()
    def select_action(self, state, deterministic=False, noise_exp=None):
        """:127-138 for a batch [N, D] -> i32[N]: argmax of the probabilities or a Categorical draw."""
        state, kind = scalar.obs_batch(state, self.device)       # ONE host observation in -> python int out (sac_cartpole.py:127-138)
        logits = self.actor.logits(state)
        if not deterministic:                        # argmax draws nothing: eval() must not move the exploration stream
            self._act_counter += 1
        act, _, _, _ = ops.categorical_sample(logits, noise_exp=noise_exp, seed=self.base_seed, counter=self._act_counter,
                                              env_id0=self.env.env_id0, deterministic=deterministic)
        return scalar.discrete_out(act, kind)

    def _eval_policy(self):
        """eval() takes the argmax of the actor's logits (the softmax does not move it)."""
        return (self.actor.fc1, self.actor.fc2, self.actor.fc3), self.actor_flat, ops.CLASSIC_HEAD_ARGMAX, 0.0

    def soft_update(self, target_flat, source_flat):
        """:140-145 on the flat parameter buffers."""
        ops.soft_update(target_flat, source_flat, self.cfg.tau)
        self._images_stale()           # a raw-pointer write: the fused step's weight images of the target are stale

    # ------------------------------------------------------------ fused vector step (csrc/dsac_step.hip) -------
    CHUNK = 16                         # vector steps per StepChunk replay (= the episode tracker's flush period)

    def _fused_update_ok(self):
        """update() as gymrl_dsac_update: opt-in (cfg.fused_step) and a matter of shapes."""
        cfg, m = self.cfg, self.memory
        return (bool(getattr(cfg, "fused_step", False))
                and ops.dsac_fused_shape_ok(cfg.batch_size, m.ring[0].shape[1], self.action_dim, cfg.hidden_dim))

    def _fused_ok(self):
        """The whole vector step fused: the update AND acting + env step + replay row (the act launch steps CartPole-v1,
        MountainCar-v0 or Acrobot-v1 itself and has no `abandon`: the trainer's own step cap must not cut an episode short)."""
        cfg, env = self.cfg, self.env
        return (self._fused_update_ok() and isinstance(env, VecEnv) and env.kind in ops.FUSED_ACT_KINDS
                and cfg.max_steps >= env.max_steps and self.memory.capacity >= env.n)

    def _fused_args(self):
        if self._fused is None or self._fused[3] is not self.env:
            cfg, env, m = self.cfg, self.env, self.memory
            D, A = m.ring[0].shape[1], self.action_dim
            img = ops.dsac_images(cfg.hidden_dim, self.device) if getattr(cfg, "fused_images", True) else None
            act = (ops.dsac_act_args(env, self.actor, m.ring, m.capacity, img)
                   if isinstance(env, VecEnv) and env.kind in ops.FUSED_ACT_KINDS else None)
            ws = ops.dsac_update_workspace(cfg.batch_size, D, A, cfg.hidden_dim, self.device)
            upd = ops.dsac_update_args(cfg.batch_size, D, A, self.actor, self.critic1, self.critic2, self.critic1_target,
                                       self.critic2_target, self.actor_optim, self.critic1_optim, self.critic2_optim, m.ring,
                                       (cfg.gamma, cfg.tau, cfg.target_entropy, cfg.lr_alpha), self.log_alpha, self._alpha_m,
                                       self._alpha_v, self._sums, self._alpha_loss, ws, img)
            self._fused = (act, upd, ws, env, img)
            self._images_stale()
        if self._fused[4] is not None:         # (flat.WeightImages: rebuilt when a parameter moved outside the fused update)
            self._refresh_images(((self.actor_flat, self.actor), (self.c1_flat, self.critic1), (self.c2_flat, self.critic2),
                                  (self.c1_target_flat, self.critic1_target), (self.c2_target_flat, self.critic2_target)),
                                 ops.dsac_pack_images, self._fused[1])
        return self._fused

    def _update_fused(self, indices=None, dev=None):
        """update() as gymrl_dsac_update's four launches.  dev = (draw, adam_c1, adam_c2, adam_a, alpha) device records of a
        StepChunk replay; None: this call's scalars travel as arguments and the host counters advance here."""
        m = self.memory
        upd = self._fused_args()[1]
        if dev is not None:
            ops.dsac_update(upd, idx_seed=m.seed, idx_dev=dev[0], idx_size=m.capacity, adam_critic1_dev=dev[1], adam_critic2_dev=dev[2],
                            adam_actor_dev=dev[3], alpha_bias_dev=dev[4])
            return
        if indices is None:
            counter, size = m.draws, m.size
            m.draws += 1
        else:
            counter, size = 0, 0
            if indices.dtype != torch.int32:
                indices = indices.to(torch.int32)
        self._alpha_steps += 1
        ops.dsac_update(upd, idx=indices, idx_seed=m.seed, idx_counter=counter, idx_size=size,
                        adam_critic1=self.critic1_optim.next_bias(), adam_critic2=self.critic2_optim.next_bias(),
                        adam_actor=self.actor_optim.next_bias(), alpha_t=self._alpha_steps)

    def _act_fused(self, lb, obs, nxt, ep_ret, done, cursor_dev=None, counter_dev=None):
        """Acting + env step + replay row of one vector step: one launch (select_action + env.step + memory.push)."""
        env, m = self.env, self.memory
        noise = None if self._parity_noise is None else next(self._parity_noise)
        if cursor_dev is None:
            self._act_counter += 1
        ops.dsac_act_step(self._fused_args()[0], env, obs, nxt, cursor=m.cursor, cursor_dev=cursor_dev, noise_exp=noise,
                          seed=self.base_seed, counter=self._act_counter, counter_dev=counter_dev,
                          rew_out=lb["rew"], done_out=done, ep_ret_out=ep_ret, ep_stats=env.ep_stats)
        if cursor_dev is None:
            m.advance(env.n)

    def _loop_buffers(self, N, D):
        """Step buffers that outlive one train() call: the captured StepChunk graph holds their addresses."""
        lb = getattr(self, "_loop", None)
        if lb is None or lb["N"] != N:
            d = self.device
            lb = self._loop = dict(N=N, obs=torch.empty(N, D, device=d), nxt=torch.empty(N, D, device=d), rew=torch.empty(N, device=d),
                                   tracker=EpisodeTracker(N, d, flush_every=1 if N == 1 else self.CHUNK))
        lb["tracker"].k, lb["tracker"].episodes = 0, 0
        return lb

    def _chunk_body(self, lb, j):
        """Vector step j of a StepChunk capture: the act launch and the update's, every per-step scalar read from record j."""
        ch, tr = self._chunk, lb["tracker"]
        obs, nxt = (lb["obs"], lb["nxt"]) if j % 2 == 0 else (lb["nxt"], lb["obs"])
        self._act_fused(lb, obs, nxt, tr.ret[j], tr.done[j], cursor_dev=ch.view(j, "push"), counter_dev=ch.view(j, "act"))
        self._update_fused(dev=(ch.view(j, "draw"), ch.view(j, "adam_c1", torch.float32), ch.view(j, "adam_c2", torch.float32),
                                ch.view(j, "adam_a", torch.float32), ch.view(j, "alpha", torch.float64)))

    def _stage_chunk(self):
        """The host's bookkeeping of the next CHUNK vector steps, in the eager loop's order, written into the records."""
        ch, m, N = self._chunk, self.memory, self.env.n
        b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))              # the kernel's float32 betas, as doubles
        for j in range(ch.K):
            ch.set(j, "push", m.cursor)
            m.advance(N)
            self._act_counter += 1
            ch.set(j, "act", self._act_counter)
            ch.set(j, "draw", m.draws, m.size)
            m.draws += 1
            self._alpha_steps += 1
            ch.set(j, "alpha", 1.0 - b1 ** self._alpha_steps, 1.0 - b2 ** self._alpha_steps)
            ch.set_bytes(j, "adam_c1", self.critic1_optim.next_bias())
            ch.set_bytes(j, "adam_c2", self.critic2_optim.next_bias())
            ch.set_bytes(j, "adam_a", self.actor_optim.next_bias())
        ch.flush()

    def _train_fused(self, max_vector_steps=None):
        """_train on the fused step.  With hipGraphs on, CHUNK whole vector steps replay as one graph (graphs.StepChunk);
        while the ring holds fewer rows than a batch — and for what a chunk cannot take — the loop is eager: the act launch,
        then the update's, no host round trip (the loss sums stay on the device)."""
        cfg, env, m = self.cfg, self.env, self.memory
        N, D = env.n, env.obs_dim
        lb = self._loop_buffers(N, D)
        obs, nxt, tracker = lb["obs"], lb["nxt"], lb["tracker"]
        env.reset(obs)
        step = 0
        pending = None            # drain_async() token of the last chunk, collected one chunk later
        graphed = bool(getattr(cfg, "use_graphs", True)) and self._parity_indices is None
        chunked = graphed and N > 1 and cfg.updates_per_step == 1 and self._parity_noise is None
        limit = max_vector_steps or (cfg.max_episodes * cfg.max_steps // N + 1)
        while tracker.episodes < cfg.max_episodes and step < limit:
            if chunked and tracker.k == 0 and limit - step >= self.CHUNK and obs is lb["obs"] and len(m) >= cfg.batch_size:
                if getattr(self, "_chunk", None) is None:
                    from .graphs import StepChunk
                    self._chunk = StepChunk(self.device, self.CHUNK, [("push", "q"), ("draw", "Qq"), ("adam_c1", "4f"), ("adam_c2", "4f"),
                                                                      ("adam_a", "4f"), ("alpha", "2d"), ("act", "Q")])
                self._fused_args()             # weight images rebuilt (if stale) BEFORE the capture, not inside it
                self._stage_chunk()
                self._chunk.run(lambda j: self._chunk_body(lb, j), key=(id(env), env.state.data_ptr()))
                step += self.CHUNK
                tracker.k = self.CHUNK
                token = tracker.drain_async()      # the chunk's episode returns come back one chunk late: the host goes on staging
                tracker.collect(pending, self.episode_rewards)
                pending = token
                if cfg.max_episodes - tracker.episodes <= N * self.CHUNK:      # within reach of the episode budget: no lag
                    tracker.collect(pending, self.episode_rewards)
                    pending = None
                continue
            tracker.collect(pending, self.episode_rewards)
            pending = None
            ep_ret, done = tracker.slot()
            self._act_fused(lb, obs, nxt, ep_ret, done)
            for _ in range(cfg.updates_per_step):
                if len(m) >= cfg.batch_size:
                    self._update_fused(None if self._parity_indices is None else next(self._parity_indices))
            obs, nxt = nxt, obs
            step += 1
            tracker.advance(self.episode_rewards)
        tracker.collect(pending, self.episode_rewards)
        tracker.flush(self.episode_rewards)
        self.env.close()

    def update(self, indices=None):
        """:148-227 -> (actor_loss, critic1_loss, critic2_loss, alpha_loss) python floats."""
        cfg = self.cfg
        if len(self.memory) < cfg.batch_size:
            return 0.0, 0.0, 0.0, 0.0
        if indices is None and self._parity_indices is not None:
            indices = next(self._parity_indices)
        if self._fused_update_ok() and (indices is None or indices.numel() == cfg.batch_size):
            self._update_fused(indices)
            s = self._sums.tolist()
            return s[2] / cfg.batch_size, s[0] / cfg.batch_size, s[1] / cfg.batch_size, float(self._alpha_loss.item())
        if indices is None:
            indices = self.memory.draw_indices(cfg.batch_size)
        B = self._update_body(indices)
        sc, sa = self._sums_c.tolist(), self._sums_a.tolist()
        return sa[0] / B, sc[0] / B, sc[1] / B, float(self._alpha_loss.item())

    def _update_body(self, indices, biases=None, alpha_bias=None):
        """Everything after the index draw; biases = device views of the three Adams' step scalars (critic1, critic2,
        actor) and alpha_bias the temperature's, when the body runs inside / ahead of a hipGraph."""
        cfg = self.cfg
        self._images_stale()                  # this path writes the parameters without the fused step's weight images
        bc1, bc2, ba = biases if biases is not None else (None, None, None)
        states, actions, rewards, next_states, dones = self.memory.gather(indices)
        B = states.shape[0]
        with torch.no_grad():                                                  # :171-181
            y = ops.dsac_target(self.actor(next_states), self.critic1_target(next_states),
                                self.critic2_target(next_states), rewards, dones, self.log_alpha, cfg.gamma)
        q1, q2 = self.critic1(states), self.critic2(states)                    # :183-194
        self._sums_c.zero_()
        dq1, dq2 = ops.dsac_critic_loss(q1.detach(), q2.detach(), actions.view(-1).to(torch.int32), y, self._sums_c)
        self._c1_sink.arm()
        self._c2_sink.arm()
        torch.autograd.backward([q1, q2], [dq1, dq2])
        self._c1_sink.collect()
        self._c2_sink.collect()
        self.critic1_optim.step(bias_dev=bc1, polyak=(self.c1_target_flat, cfg.tau))             # + soft updates :217-218
        self.critic2_optim.step(bias_dev=bc2, polyak=(self.c2_target_flat, cfg.tau))
        probs = self.actor(states)                                             # :196-207
        with torch.no_grad():
            q1n, q2n = self.critic1(states), self.critic2(states)              # the critics' gradients of this loss are discarded
        self._sums_a.zero_()
        dprobs = ops.dsac_actor_loss(probs.detach(), q1n, q2n, self.log_alpha, self._sums_a)
        self._actor_sink.arm()
        torch.autograd.backward([probs], [dprobs])
        self._actor_sink.collect()
        self.actor_optim.step(bias_dev=ba)
        if alpha_bias is None:                                                 # :209-215
            self._alpha_steps += 1
        ops.dsac_alpha_step(self.log_alpha, self._alpha_m, self._alpha_v, self._sums_a, B, cfg.target_entropy,
                            cfg.lr_alpha, max(self._alpha_steps, 1), loss_out=self._alpha_loss, bias_dev=alpha_bias)
        return B

    def update_async(self):
        """update() without the host round trip, replayed as a captured hipGraph (gymrl_amd/graphs.py)."""
        cfg = self.cfg
        if len(self.memory) < cfg.batch_size:
            return
        if self._fused_update_ok():        # four launches: nothing left for a graph to save
            return self._update_fused()
        if self._graph is None:
            from .graphs import GraphedUpdate
            b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))          # the kernel's float32 betas, as doubles
            self._graph = GraphedUpdate(self.device, cfg.batch_size, [self.critic1_optim, self.critic2_optim, self.actor_optim],
                                        lambda idx, biases, ab: self._update_body(idx, biases, ab),
                                        alpha=(self, "_alpha_steps", b1, b2))
        self._images_stale()                  # (a replay runs no Python: _update_body's own reset is not enough)
        self._graph(self.memory, cfg.batch_size)

    def save_checkpoint(self, path, include_memory=True):
        """ModelLoader-style dict: five networks, the three optimisers in torch.optim.Adam's layout, the
        float32 temperature with its Adam state, the host counters and — unlike the reference, which skips `memory` — the
        replay ring."""
        from .utils import checkpoint
        extra = {"memory_state_dict": self.memory.state_dict()} if include_memory else {}
        return checkpoint.save_agent(path, {k: getattr(self, k) for k in ("actor", "critic1", "critic2", "critic1_target", "critic2_target")},
                                     {"actor_optim": (self.actor, self.actor_optim), "critic1_optim": (self.critic1, self.critic1_optim),
                                      "critic2_optim": (self.critic2, self.critic2_optim)},
                                     log_alpha=self.log_alpha.detach().cpu(), alpha_m=self._alpha_m.cpu(), alpha_v=self._alpha_v.cpu(),
                                     alpha_steps=self._alpha_steps, _act_counter=self._act_counter,
                                     episode_rewards=list(self.episode_rewards), **extra)

    def load_checkpoint(self, path):
        from .utils import checkpoint
        rest = checkpoint.load_agent(path, {k: getattr(self, k) for k in ("actor", "critic1", "critic2", "critic1_target", "critic2_target")},
                                     {"actor_optim": (self.actor, self.actor_optim), "critic1_optim": (self.critic1, self.critic1_optim),
                                      "critic2_optim": (self.critic2, self.critic2_optim)})
        self._images_stale()                  # the fused step's weight images are rebuilt from the loaded parameters
        self.log_alpha.copy_(rest["log_alpha"].to(self.device))
        self._alpha_m.copy_(rest["alpha_m"].to(self.device))
        self._alpha_v.copy_(rest["alpha_v"].to(self.device))
        self._alpha_steps, self._act_counter = int(rest["alpha_steps"]), int(rest["_act_counter"])
        self.episode_rewards.clear()
        self.episode_rewards.extend(rest.get("episode_rewards", []))
        if "memory_state_dict" in rest:
            self.memory.load_state_dict(rest["memory_state_dict"])
        return rest

    def train(self, max_vector_steps=None):
        """The reference's train() loop (every Linear of the update and of acting is a gymrl_lin_* launch: gymrl_amd/nn.py)."""
        return self._train(max_vector_steps)

    def _train(self, max_vector_steps=None):
        """:229-262 with N lock-stepped envs."""
        cfg, env = self.cfg, self.env
        if self._fused_ok():
            return self._train_fused(max_vector_steps)
        N, D = env.n, env.obs_dim
        obs, nxt, tobs = (torch.empty(N, D, device=self.device) for _ in range(3))
        rew = torch.empty(N, device=self.device)
        tracker = EpisodeTracker(N, self.device, flush_every=1 if N == 1 else 16)
        env.reset(obs)
        step = 0
        graphed = bool(getattr(cfg, "use_graphs", True)) and self._parity_indices is None
        limit = max_vector_steps or (cfg.max_episodes * cfg.max_steps // N + 1)
        while tracker.episodes < cfg.max_episodes and step < limit:
            action = self.select_action(obs, noise_exp=None if self._parity_noise is None else next(self._parity_noise))
            ep_ret, done = tracker.slot()
            env.step(action, nxt, rew, done_out=done, term_obs_out=tobs, ep_ret_out=ep_ret)
            self.memory.push(obs, action, rew, tobs, done)
            if cfg.max_steps < env.max_steps:       # the reference's `for step in range(cfg.max_steps)`: abandoned, no done flag
                env.abandon(cfg.max_steps, nxt, done, ep_ret)
            for _ in range(cfg.updates_per_step):
                if graphed:
                    self.update_async()
                else:
                    self.update()
            obs, nxt = nxt, obs
            step += 1
            tracker.advance(self.episode_rewards)
        tracker.flush(self.episode_rewards)
        self.env.close()

    @torch.no_grad()
    def eval(self, num_episodes=10):
        fused = self._eval_fused(num_episodes)
        if fused is not None:
            return fused
        env = VecEnv(self.cfg.env_name, num_episodes, device=self.device, seed=self.base_seed + 999, env_id0=1 << 40)
        obs = env.reset()
        nxt = torch.empty_like(obs)
        rew = torch.empty(num_episodes, device=self.device)
        done = torch.zeros(num_episodes, dtype=torch.uint8, device=self.device)
        ep_ret = torch.zeros(num_episodes, device=self.device)
        result = torch.full((num_episodes,), float("nan"), device=self.device)
        for _ in range(env.max_steps + 1):
            act = self.select_action(obs, deterministic=True)
            env.step(act, nxt, rew, done_out=done, ep_ret_out=ep_ret)
            result = torch.where(done.bool() & torch.isnan(result), ep_ret, result)
            obs, nxt = nxt, obs
            if not torch.isnan(result).any():
                break
        return result.tolist()

    def test(self):
        return self.eval(num_episodes=5)


if __name__ == "__main__":       # python -m gymrl_amd.sac_cartpole [--<Config attribute> <value> ...]  (sac_cartpole.py:313-329)
    from .utils.cli import run_script
    run_script(Config, SACTrainer)

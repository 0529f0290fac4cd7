"""Evaluation of a trainer's policy as whole episodes in ONE launch (csrc/eval_classic.hip; csrc/eval_duel.hip, §4q;
csrc/eval_net.hip, §4t and §4y; what an env is to all of them: §4aa).

The reference's eval() (dqn_cartpole.py:214-235 and its siblings) plays num_episodes episodes one after another under
select_action(deterministic=True).  The trainers here play them side by side on a VecEnv, one host iteration per env step;
with Config.fused_eval the same episodes — the same start draws, the same actions, the same returns — are one kernel
launch.  Four entry points serve nine trainers:

  gymrl_classic_policy_eval   a three-layer MLP: CartPole-v1 under an argmax head (DQN, DDQN+PER, discrete SAC), Pendulum-v1 under
                              a tanh head (TD3, DDPG; SAC-Pendulum's tanh(mean(fc2(fc1 s))) * bound through evaluate() only:
                              its eval() applies torch.tanh, which is not the kernels' tanh bit for bit, and keeps the loop)
  gymrl_classic_duel_eval     a dueling network on CartPole-v1: trunk -> value + advantage heads -> q = v + (a - mean a) -> the
                              first maximum (dueling DDQN+PER: one hidden layer; NoisyNet dueling DQN and Rainbow: two, the noisy
                              layers at their weight_mu / bias_mu — no noise is drawn and no draw counter moves)
  gymrl_mountaincar_net_eval  MountainCar-v0 (env_name = "MountainCar-v0") under either network: the six CartPole trainers above,
                              three-layer ones as net 0, dueling ones with the combine their trainer declares in
                              EVAL_DUEL_COMBINE — 1: torch's mean, sum * (1 / 3) (dueling DDQN+PER, NoisyNet); 2: the layer
                              kernels' DUELING epilogue, sum / 3 (Rainbow).  With three actions the two are different floats
  gymrl_acrobot_net_eval      Acrobot-v1 (env_name = "Acrobot-v1"): the same six trainers, the same three nets, (D, A) = (6, 3)

Every shape the entry points refuse (hidden 260, another action count) keeps the loop.  LunarLander-v3 has a
launch of its own on the two PPO trainers themselves (csrc/eval_lunar.hip, DESIGN §4r: other streams, a float64 return, a
population packed per policy), not through this mixin."""
import torch

from . import ops


class PolicyEval:
    """Mixin of the nine trainers.  A trainer says which layers act greedily — _eval_policy() for a three-layer MLP,
    _eval_duel_policy() for a dueling network; eval() asks _eval_fused() first and plays its loop where that returns None."""
    EVAL_SEED_OFFSET = 999             # eval()'s env streams: seed base_seed + 999, env ids from 1 << 40
    EVAL_ENV_ID0 = 1 << 40
    EVAL_DUEL_COMBINE = 1              # how the trainer's own forward takes the dueling mean (gymrl_mountaincar_net_eval's net): 1
    #                                    torch's advantage.mean(), 2 the GYMRL_ACT_DUELING epilogue of the layer kernels

    def _eval_policy(self):
        """-> ((fc1, fc2, fc3), flat parameter buffer, head, action bound), or None: no such policy."""
        return None

    def _eval_duel_policy(self):
        """-> (trunk: one or two (weight, bias) pairs, the value head's pair, the advantage head's pair, flat parameter buffer),
        or None: no dueling policy.  Asked only where _eval_policy() answers None."""
        return None

    def _eval_call(self):
        """The launch's fixed arguments — ops.classic_policy_eval's, ops.classic_duel_eval's (`trunk` is among them) or, on
        MountainCar-v0 and Acrobot-v1, ops.mountaincar_net_eval's / ops.acrobot_net_eval's (`net` is among them) — or None where the entry points would refuse the shape."""
        kind = ops.ENV_KINDS.get(self.cfg.env_name)
        if kind is None:
            return None
        if kind in (ops.MOUNTAINCAR, ops.ACROBOT):
            return self._eval_call_net(kind)
        pol = self._eval_policy()
        if pol is not None:
            (fc1, fc2, fc3), flat, head, bound = pol
            H, D, A = fc1.weight.shape[0], fc1.weight.shape[1], fc3.weight.shape[0]
            if not ops.classic_eval_shape_ok(kind, head, D, A, H):
                return None
            return dict(kind=kind, layers=(fc1, fc2, fc3), cap=ops.EPISODE_ENVS[kind][4], head=head, bound=bound, flat=flat)
        duel = self._eval_duel_policy()
        if duel is None:
            return None
        trunk, value, advantage, flat = duel
        (H, D), A = trunk[0][0].shape, advantage[0].shape[0]
        if not ops.classic_duel_eval_shape_ok(kind, len(trunk), D, A, H):
            return None
        return dict(kind=kind, trunk=trunk, value=value, advantage=advantage, cap=ops.EPISODE_ENVS[kind][4], flat=flat)

    def _eval_call_net(self, kind):
        """_eval_call() on MountainCar-v0 / Acrobot-v1: a three-layer policy is net 0, a dueling one the combine the trainer
        declares.  The call is the keyword arguments of the env's own wrapper, so only Acrobot-v1's carries `kind`."""
        pair = lambda m: (m.weight, m.bias)     # noqa: E731
        pol = self._eval_policy()
        if pol is not None:
            (fc1, fc2, fc3), flat, head, _ = pol
            if head != ops.CLASSIC_HEAD_ARGMAX:
                return None
            net, trunk, top, value = ops.MOUNTAINCAR_NET_MLP, [pair(fc1), pair(fc2)], pair(fc3), None
        else:
            duel = self._eval_duel_policy()
            if duel is None:
                return None
            trunk, value, top, flat = duel
            net = self.EVAL_DUEL_COMBINE
        (H, D), A = trunk[0][0].shape, top[0].shape[0]
        if not ops.net_eval_shape_ok(kind, net, len(trunk), D, A, H):
            return None
        call = dict(net=net, trunk=trunk, head=top, value=value, cap=ops.EPISODE_ENVS[kind][4], flat=flat)
        return dict(call, kind=kind) if kind == ops.ACROBOT else call

    @staticmethod
    def _eval_launch(call, **kw):
        """One launch of the wrapper the call's keyword arguments are of.  A call is nothing but those arguments — callers hand it,
        or a dict rebuilt from it, to the wrapper themselves — so the wrapper is read off the names it uses."""
        fn = (ops.acrobot_net_eval if call.get("kind") == ops.ACROBOT and "net" in call else
              ops.mountaincar_net_eval if "net" in call else ops.classic_duel_eval if "trunk" in call else ops.classic_policy_eval)
        return fn(**kw, **call)

    def _eval_fused(self, num_episodes):
        """eval(num_episodes) as one launch -> the list the loop returns, or None: fused_eval is off or the shape is refused.
        Neither the exploration or noise counters, nor self.env, nor the replay ring are touched."""
        if not getattr(self.cfg, "fused_eval", False) or num_episodes < 1:
            return None
        call = self._eval_call()
        if call is None:
            return None
        returns, _, _ = self._eval_launch(call, n_episodes=num_episodes, seed=self.base_seed + self.EVAL_SEED_OFFSET,
                                          stream_id0=self.EVAL_ENV_ID0)
        return returns[0].tolist()

    @torch.no_grad()
    def evaluate(self, num_episodes, params=None, stream_offset=0):
        """-> (returns f32, lengths i32, terminated u8), numpy arrays [P, num_episodes]: whole episodes on eval()'s streams
        (episode e: seed base_seed + 999, env id (1 << 40) + stream_offset + e), every policy from the same starts, in one
        launch whatever Config.fused_eval says.  params = None: the trainer's own policy (P = 1); params = f32[P, n]: a stack of
        flat parameter buffers in the layout of the trainer's own.  Raises where the entry points take no such policy."""
        call = self._eval_call()
        if call is None:
            raise RuntimeError(f"{type(self).__name__}.evaluate: gymrl_classic_policy_eval / gymrl_classic_duel_eval / "
                               "gymrl_mountaincar_net_eval / gymrl_acrobot_net_eval take no such policy (include/gymrl.h)")
        if params is not None:
            params = torch.as_tensor(params, dtype=torch.float32).to(self.device)
            params = params.view(1, -1) if params.dim() == 1 else params.contiguous()
        out = self._eval_launch(call, n_episodes=num_episodes, seed=self.base_seed + self.EVAL_SEED_OFFSET,
                                stream_id0=self.EVAL_ENV_ID0 + int(stream_offset), params=params)
        return tuple(t.cpu().numpy() for t in out)

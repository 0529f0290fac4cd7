"""Evaluation of a trainer's policy as whole episodes in ONE launch (csrc/eval_classic.hip).

The reference's eval() (dqn_cartpole.py:214-235 and its siblings) plays num_episodes episodes one after another under
select_action(deterministic=True).  The trainers here play them side by side on a VecEnv, one host iteration per env step;
with Config.fused_eval the same episodes — the same start draws, the same actions, the same returns — are one kernel
launch.  CartPole-v1 under an argmax head (DQN, DDQN+PER, discrete SAC) and Pendulum-v1 under a tanh head (TD3, DDPG); not
the dueling, NoisyNet, Rainbow or SAC-Pendulum heads, MountainCar-v0 or LunarLander-v3: those trainers keep the loop."""
import torch

from . import ops


class PolicyEval:
    """Mixin of the five trainers.  A trainer says which three layers act greedily (_eval_policy); eval() asks _eval_fused()
    first and plays its loop where that returns None."""
    EVAL_SEED_OFFSET = 999             # eval()'s env streams: seed base_seed + 999, env ids from 1 << 40
    EVAL_ENV_ID0 = 1 << 40

    def _eval_policy(self):
        """-> ((fc1, fc2, fc3), flat parameter buffer, head, action bound), or None: no such policy."""
        return None

    def _eval_call(self):
        """The launch's fixed arguments, or None where the entry point would refuse the shape."""
        pol = self._eval_policy()
        kind = ops.ENV_KINDS.get(self.cfg.env_name)
        if pol is None or kind is None:
            return None
        (fc1, fc2, fc3), flat, head, bound = pol
        H, D, A = fc1.weight.shape[0], fc1.weight.shape[1], fc3.weight.shape[0]
        if not ops.classic_eval_shape_ok(kind, head, D, A, H):
            return None
        return dict(kind=kind, layers=(fc1, fc2, fc3), cap=ops.env_dims(kind)[3], head=head, bound=bound, flat=flat)

    def _eval_fused(self, num_episodes):
        """eval(num_episodes) as one launch -> the list the loop returns, or None: fused_eval is off or the shape is refused.
        Neither the exploration counters, nor self.env, nor the replay ring are touched."""
        if not getattr(self.cfg, "fused_eval", False) or num_episodes < 1:
            return None
        call = self._eval_call()
        if call is None:
            return None
        returns, _, _ = ops.classic_policy_eval(n_episodes=num_episodes, seed=self.base_seed + self.EVAL_SEED_OFFSET,
                                                stream_id0=self.EVAL_ENV_ID0, **call)
        return returns[0].tolist()

    @torch.no_grad()
    def evaluate(self, num_episodes, params=None, stream_offset=0):
        """-> (returns f32, lengths i32, terminated u8), numpy arrays [P, num_episodes]: whole episodes on eval()'s streams
        (episode e: seed base_seed + 999, env id (1 << 40) + stream_offset + e), every policy from the same starts, in one
        launch whatever Config.fused_eval says.  params = None: the trainer's own policy (P = 1); params = f32[P, n]: a stack of
        flat parameter buffers in the layout of the trainer's own.  Raises where the entry point takes no such policy."""
        call = self._eval_call()
        if call is None:
            raise RuntimeError(f"{type(self).__name__}.evaluate: gymrl_classic_policy_eval takes no such policy (include/gymrl.h)")
        if params is not None:
            params = torch.as_tensor(params, dtype=torch.float32).to(self.device)
            params = params.view(1, -1) if params.dim() == 1 else params.contiguous()
        out = ops.classic_policy_eval(n_episodes=num_episodes, seed=self.base_seed + self.EVAL_SEED_OFFSET,
                                      stream_id0=self.EVAL_ENV_ID0 + int(stream_offset), params=params, **call)
        return tuple(t.cpu().numpy() for t in out)

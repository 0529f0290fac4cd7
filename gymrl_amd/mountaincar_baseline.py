"""Hand-crafted rule baseline for MountainCar-v0 — MI355X engine behind the reference's algorithms/mountaincar_baseline.py
surface: Config :19-23, RuleBasedAgent :26-91 (select_action :35-45, run_episode :47-68, eval :70-84, test :86-91).

There is nothing to train: the script only evaluates.  eval() / evaluate() are csrc/mountaincar.hip's
gymrl_mountaincar_rule_eval: one lane per (policy, episode), whole episodes in ONE launch, nothing but the results copied back;
evaluate() also takes a population of coefficient sets [P, 9] for the rule.  run_episode() is the reference's loop over the
single-env view of a device-resident env (envs.GymView: one launch and one small copy per step) for callers written against it.

The rule is evaluated in float64 on the float32 observation with powers as products (include/gymrl.h): the reference's own
expression runs in float32 or float64 depending on the NumPy under it, and the float64 form agrees with both wherever the
observation is not within rounding distance of a boundary (tests/test_mountaincar_ref.py).

One deliberate departure: the reference resets every evaluation episode with seed = 42, so its ten episodes are one episode
ten times; here evaluation episode e has its own start draw, stream (1 << 40) + e.  run_episode() keeps the reference's
reset(seed=cfg.seed) and is therefore the same episode every time, as there.  There is no renderer: test() reports one more
episode where the reference renders one.
"""
import numpy as np
import torch

from . import ops
from .envs import VecEnv
from .tabular import EVAL_STREAM0, VISUAL_STREAM_OFFSET


class Config:
    def __init__(self):
        self.env_name = "MountainCar-v0"
        self.seed = 42
        self.test_episodes = 10
        # --- engine additions ---
        self.device = "cuda"
        self.episode_cap = 200               # steps after which an evaluation episode is cut (1..200, the env's TimeLimit)


class RuleBasedAgent:
    coefs = ops.MOUNTAINCAR_RULE_COEFS

    def __init__(self, config: Config):
        self.cfg = config
        if not torch.cuda.is_available() or not ops.device_ok():
            raise RuntimeError("gymrl_amd.mountaincar_baseline.RuleBasedAgent needs an MI355X and libgymrl_hip.so; no CPU fallback")
        self.device = torch.device(config.device)
        # env 0 of this vector is evaluation stream 0: run_episode() is evaluate(1)'s episode
        self.env = VecEnv(config.env_name, 1, device=self.device, seed=config.seed, env_id0=EVAL_STREAM0)

        print(f"Environment: {config.env_name}")
        print("Observation space: Box([-1.2 -0.07], [0.6 0.07], (2,), float32)")
        print(f"Action space: Discrete({self.env.action_space.n})")

    def select_action(self, observation) -> int:
        k = self.coefs
        position, velocity = float(np.float32(observation[0])), float(np.float32(observation[1]))
        a = position + k[1]
        l1 = k[0] * (a * a) + k[2]
        b = position + k[4]
        b2 = b * b
        l2 = k[3] * (b2 * b2) - k[5]
        lb = l1 if l1 < l2 else l2
        c = position + k[7]
        ub = k[6] * (c * c) + k[8]
        if lb < velocity < ub:
            return 2
        else:
            return 0

    def run_episode(self, render: bool = False):
        if render:
            raise NotImplementedError("gymrl_amd has no renderer: test() reports one more episode instead")
        env = self.env.gym

        state, _ = env.reset(seed=self.cfg.seed)
        episode_reward = 0.0
        done = False
        steps = 0

        while not done:
            action = self.select_action(state)
            state, reward, terminated, truncated, _ = env.step(action)
            done = terminated or truncated
            episode_reward += reward
            steps += 1

        return episode_reward, steps

    def evaluate(self, num_episodes, coefs=None, stream_offset=0):
        """(returns, lengths, reached) of num_episodes episodes per policy, numpy [P, num_episodes]; coefs [P, 9] (or [9]) are
        the rule's constants, None: this agent's.  One launch.  stream_offset moves the start draws to another block of streams."""
        if coefs is None and self.coefs != ops.MOUNTAINCAR_RULE_COEFS:
            coefs = self.coefs
        if coefs is not None:
            coefs = torch.from_numpy(np.ascontiguousarray(np.atleast_2d(np.asarray(coefs, np.float64)))).to(self.device)
        out = ops.mountaincar_rule_eval(int(num_episodes), self.cfg.seed, EVAL_STREAM0 + stream_offset, int(self.cfg.episode_cap),
                                        self.device, coefs=coefs)
        return tuple(t.cpu().numpy() for t in out)

    def eval(self, num_episodes: int = 10) -> list:
        print(f"\nEvaluating for {num_episodes} episodes...")
        returns, lengths, _ = self.evaluate(num_episodes)
        rewards, steps_list = returns[0].tolist(), lengths[0].tolist()

        for episode in range(num_episodes):
            print(f"  Episode {episode + 1}: Reward = {rewards[episode]:.0f}, Steps = {steps_list[episode]}")

        print(f"Evaluation: Mean Reward = {np.mean(rewards):.1f}, Mean Steps = {np.mean(steps_list):.1f}")
        return rewards

    def test(self):
        self.eval(num_episodes=self.cfg.test_episodes)

        print("\nStarting visual test...")                 # one more episode, reported instead of rendered
        returns, lengths, _ = self.evaluate(1, stream_offset=VISUAL_STREAM_OFFSET)
        print(f"Visual Test: Reward = {returns[0, 0]:.0f}, Steps = {int(lengths[0, 0])}")


if __name__ == "__main__":
    import signal
    import sys

    from .utils.cli import apply_overrides

    config = apply_overrides(Config(), sys.argv[1:])
    agent = RuleBasedAgent(config)

    def signal_handler(signum, frame):
        print("\n\nInterrupted.")
        sys.exit(0)

    signal.signal(signal.SIGINT, signal_handler)

    agent.test()

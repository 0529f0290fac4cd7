"""Evolution strategies (OpenAI-ES, or separable NES under Config.method = "snes") on the one-launch population evaluators — an engine addition with no reference script
behind it; Config / trainer / CLI are shaped like dqn_cartpole.py's.

One generation is four launches and no host synchronisation:

    OpenAIES.ask()        gymrl_es_perturb     the centre -> P mirrored policies, f32[P, stride]
    PolicyEval launch     gymrl_classic_policy_eval | gymrl_mountaincar_net_eval | gymrl_acrobot_net_eval     P policies x E whole episodes
    OpenAIES.tell()       gymrl_es_shape_grad  returns -> centred ranks -> search gradient (two launches above 256 policies)
                          gymrl_adam_step      the centre moves

Under Config.method = "snes" the learner is es.SeparableNES: gymrl_snes_perturb, the same evaluation launch, and
gymrl_snes_tell, which moves the centre and its per-element step sizes itself — three launches, no Adam step; Config.sigma is
the step sizes' initial value and Config.lr is not read.

The policy is dqn_cartpole.py's three-layer MLP: an argmax head on CartPole-v1, MountainCar-v0 and Acrobot-v1, tanh(fc3) * bound on
Pendulum-v1.  Training episodes start from streams of their own (env ids from 1 << 41, E fresh ones per generation, the same E
for every policy of a generation), so no training start is an eval() start."""
import time

import torch

from . import ops
from .dqn_cartpole import QNetwork
from .envs import VecEnv
from .es import OpenAIES, SeparableNES
from .flat import flatten_module
from .policy_eval import PolicyEval
from .utils import scalar


class Config:
    def __init__(self):
        self.env_name = "CartPole-v1"        # | "Pendulum-v1" | "MountainCar-v0" | "Acrobot-v1"
        self.seed = None
        self.hidden_dim = 64
        self.population = 256                # even: population / 2 mirrored pairs
        self.sigma = 0.1
        self.lr = 0.03
        self.method = "openai"               # | "snes": es.SeparableNES, a step size per parameter adapted by the learner's own launch
        self.eta_mu = 1.0                    # "snes": the centre's learning rate
        self.eta_sigma = None                # "snes": the step sizes' learning rate; None: (3 + ln n) / (5 sqrt n)
        self.episodes_per_policy = 16        # a workgroup of the evaluators carries 16 episodes: up to here they cost no launch time
        self.max_generations = 100
        self.log_freq = 10                   # generations between host reads of the mean population return
        self.device = "cuda"
        self.fused_eval = True               # eval() as ONE launch (csrc/eval_classic.hip); off: the step-by-step loop


def make_learner(config, flat_params, seed):
    """The learner Config.method names, on the trainer's flat buffer."""
    if config.method == "openai":
        return OpenAIES(flat_params, seed, config.population, config.sigma, config.lr)
    if config.method == "snes":
        return SeparableNES(flat_params, seed, config.population, config.sigma, eta_mu=config.eta_mu, eta_sigma=config.eta_sigma)
    raise ValueError(f"ESTrainer: method is 'openai' or 'snes', not {config.method!r}")


def check_method(rest, method):
    """A checkpoint's learner state fits the learner that wrote it only (one written before there was a choice: OpenAI-ES's)."""
    saved = rest.get("method", "openai")
    if saved != method:
        raise ValueError(f"ESTrainer: the checkpoint holds a {saved!r} learner, this trainer runs {method!r}")


class ESTrainer(PolicyEval):
    TRAIN_ENV_ID0 = 1 << 41                  # training streams: env ids TRAIN_ENV_ID0 + generation * E + e (eval(): from 1 << 40)

    def __init__(self, config):
        self.cfg = config
        if not torch.cuda.is_available() or not ops.device_ok():
            raise RuntimeError("gymrl_amd.ESTrainer needs an MI355X and libgymrl_hip.so; no CPU fallback")
        self.device = torch.device(config.device if ":" in str(config.device) else f"cuda:{torch.cuda.current_device()}")
        self.base_seed = 0 if config.seed is None else int(config.seed)
        kind = ops.ENV_KINDS.get(config.env_name)
        if kind not in (ops.CARTPOLE, ops.PENDULUM, ops.MOUNTAINCAR, ops.ACROBOT):
            raise ValueError(f"ESTrainer: no population evaluator for {config.env_name!r}")
        state_dim, action_dim, self.discrete, _ = ops.env_dims(kind)
        self.action_bound = 2.0 if kind == ops.PENDULUM else 0.0          # Pendulum-v1's max torque
        g = torch.random.get_rng_state()
        torch.manual_seed(self.base_seed)
        self.policy_net = QNetwork(state_dim, action_dim, config.hidden_dim)
        torch.random.set_rng_state(g)
        self.flat_params, _ = flatten_module(self.policy_net, self.device)
        self.es = make_learner(config, self.flat_params, self.base_seed)
        self._call = self._eval_call()
        if self._call is None:
            raise ValueError(f"ESTrainer: the evaluators take no {config.env_name} policy of hidden width {config.hidden_dim} "
                             "(include/gymrl.h)")
        self.last_returns = None             # f32[P, E] on the device: what the last generation's launch returned
        self.history = []                    # (generation, mean population return) at the logged generations

    def _eval_policy(self):
        net = self.policy_net.net
        head = ops.CLASSIC_HEAD_ARGMAX if self.discrete else ops.CLASSIC_HEAD_TANH
        return (net[0], net[2], net[4]), self.flat_params, head, self.action_bound

    @property
    def generation(self):
        return self.es.generation

    def train_stream_id0(self, generation=None):
        g = self.es.generation if generation is None else generation
        return self.TRAIN_ENV_ID0 + g * self.cfg.episodes_per_policy

    @torch.no_grad()
    def step_generation(self):
        """ask -> the evaluators' launch -> tell: four launches, nothing read back."""
        stack = self.es.ask()
        returns, _, _ = self._eval_launch(self._call, n_episodes=self.cfg.episodes_per_policy,
                                          seed=self.base_seed + self.EVAL_SEED_OFFSET, stream_id0=self.train_stream_id0(),
                                          params=stack)
        self.es.tell(returns)
        self.last_returns = returns

    def train(self, max_generations=None):
        cfg = self.cfg
        last = cfg.max_generations if max_generations is None else self.es.generation + max_generations
        t0 = time.time()
        while self.es.generation < last:
            self.step_generation()
            g = self.es.generation
            if cfg.log_freq > 0 and (g % cfg.log_freq == 0 or g == last):
                mean = float(self.last_returns.mean().item())          # the loop's only host read
                self.history.append((g, mean))
                print(f"generation {g}  mean population return {mean:.2f}  ({time.time() - t0:.1f} s)")
        return self.history

    @torch.no_grad()
    def select_action(self, state, deterministic=True):
        """The centre's greedy action for a batch [N, D] (ES explores in parameter space: there is no other kind)."""
        state, kind = scalar.obs_batch(state, self.device)
        out = self.policy_net(state)
        if self.discrete:
            return scalar.discrete_out(ops.epsilon_greedy(out, 0.0, seed=self.base_seed, counter=0, env_id0=0), kind)
        return scalar.continuous_out(torch.tanh(out) * self.action_bound, kind)

    @torch.no_grad()
    def eval(self, num_episodes=10):
        fused = self._eval_fused(num_episodes)
        if fused is not None:
            return fused
        env = VecEnv(self.cfg.env_name, num_episodes, device=self.device, seed=self.base_seed + self.EVAL_SEED_OFFSET,
                     env_id0=self.EVAL_ENV_ID0)
        obs = env.reset()
        nxt = torch.empty_like(obs)
        rew = torch.empty(num_episodes, device=self.device)
        done = torch.zeros(num_episodes, dtype=torch.uint8, device=self.device)
        ep_ret = torch.zeros(num_episodes, device=self.device)
        result = torch.full((num_episodes,), float("nan"), device=self.device)
        for _ in range(env.max_steps + 1):
            act = self.select_action(obs)
            env.step(act.contiguous(), nxt, rew, done_out=done, ep_ret_out=ep_ret)
            result = torch.where(done.bool() & torch.isnan(result), ep_ret, result)
            obs, nxt = nxt, obs
            if not torch.isnan(result).any():
                break
        return result.tolist()

    def test(self):
        returns = self.eval(num_episodes=5)
        print(f"test: mean return {sum(returns) / len(returns):.2f} over {len(returns)} episodes")
        return returns

    def save_checkpoint(self, path):
        from .utils import checkpoint
        return checkpoint.save_agent(path, {"policy_net": self.policy_net}, {}, es_state_dict=self.es.state_dict(),
                                     generation=self.es.generation, history=list(self.history), method=self.cfg.method)

    def load_checkpoint(self, path):
        from .utils import checkpoint
        rest = checkpoint.load_agent(path, {"policy_net": self.policy_net}, {})
        check_method(rest, self.cfg.method)
        self.es.load_state_dict(rest["es_state_dict"])
        self.history = [tuple(h) for h in rest.get("history", [])]
        return rest


if __name__ == "__main__":       # python -m gymrl_amd.es_cartpole [--<Config attribute> <value> ...]
    from .utils.cli import run_script
    run_script(Config, ESTrainer)

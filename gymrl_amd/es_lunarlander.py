"""Evolution strategies on LunarLander-v3 (separable NES by default, OpenAI-ES under Config.method = "openai") — an engine
addition with no reference script behind it; Config / trainer / CLI are shaped like es_cartpole.py's.

The policy is ppo_lunarlander.py's ActorCritic at Config.hidden_dim, flattened as PPOTrainer flattens it (ppo_net.LAYOUT), so
that the learner's population buffer f32[P, stride] is a stack of PPO flat parameter vectors: ops.LunarPolicyStack packs it and
gymrl_lunar_policy_eval plays P policies x E whole episodes in ONE launch.  The learner perturbs and moves the whole buffer: the
critic (no evaluator reads a value) and the alignment gaps (no layer reads them) drift like everything else and are read by
nobody.  There is no rollout buffer, no optimiser over gradients and no env object.

One generation (no host synchronisation, no allocation of the stack: the trainer keeps one for the run):

    learner.ask()               gymrl_snes_perturb | gymrl_es_perturb     the centre -> P mirrored policies
    ops.LunarPolicyStack        gymrl_mlp_pack_stack, ONE launch          the stack in the one-launch forward's weight layout
    ops.lunar_policy_eval       gymrl_lunar_policy_eval                   returns f64[P, E]
    learner.tell()              "snes":   gymrl_snes_tell on the float64 returns as they are
                                "openai": one .to(torch.float32) launch, gymrl_es_shape_grad, gymrl_adam_step — its fitness
                                          is the sum of the CASTS, not the cast of the float64 sum

Training episodes start from streams of their own (seed base_seed + 1_000_003, env ids from 1 << 41, E fresh ones per
generation, the same E for every policy of a generation: common random numbers), so no training start is an eval() start
(env ids from 1 << 40).

Config.policy = "mlprnn" searches the recurrent policy instead: ppg_rnn_lunarlander.py's PSCN -> MLPRNN -> heads network at the
one width gymrl_lunar_mlprnn_eval takes (Config.hidden_dim is not read), flattened in PPGTrainer's order (critic, trunk, auxiliary
critic).  That evaluator reads flat parameter vectors as they are, so there is NO packing launch and no copy: ops.MlprnnPolicyStack
(copy=False) describes the learner's population buffer where it lies and a generation is ask, evaluate, tell.  Every episode
starts from the hidden state 0.  The observations are read RAW (norm_stats = None): an ES run keeps no running statistics, so a
policy found here is not PPGTrainer's, which normalises — its checkpoint carries the network under a key of its own
(`es_net_state_dict`) and its `policy`, and a file of the other policy is refused."""
import time

import torch

from . import ops, ppo_net
from .es_cartpole import check_method, make_learner
from .flat import flatten_module
from .ppo_lunarlander import ActorCritic

POLICIES = ("mlp", "mlprnn")


def check_policy(rest, policy):
    """A checkpoint's network and learner state fit the policy that wrote them only (one written before there was a choice:
    the feed-forward one's)."""
    saved = rest.get("policy", "mlp")
    if saved != policy:
        raise ValueError(f"es_lunarlander.ESTrainer: the checkpoint holds a {saved!r} policy, this trainer searches {policy!r}")


class Config:
    def __init__(self):
        self.env_name = "LunarLander-v3"
        self.seed = None
        self.policy = "mlp"                  # | "mlprnn": the recurrent PSCN -> MLPRNN -> heads network, raw observations
        self.hidden_dim = 64                 # "mlp" only
        self.method = "snes"                 # | "openai"
        self.population = 256                # even: population / 2 mirrored pairs
        self.sigma = 0.1                     # "snes": the initial step size of every parameter
        self.eta_mu = 1.0                    # "snes": the centre's learning rate
        self.eta_sigma = None                # "snes": the step sizes' learning rate; None: (3 + ln n) / (5 sqrt n)
        self.lr = 0.03                       # "openai": Adam's
        self.episodes_per_policy = 16        # a workgroup of the evaluator carries 16 episodes
        self.max_generations = 100
        self.log_freq = 10                   # generations between host reads of the mean population return
        self.device = "cuda"


class ESTrainer:
    EVAL_SEED_OFFSET, EVAL_ENV_ID0 = 1_000_003, 1 << 40      # PPOTrainer's: eval()'s env streams
    TRAIN_ENV_ID0 = 1 << 41                                  # training streams: env ids TRAIN_ENV_ID0 + generation * E + e

    def __init__(self, config):
        self.cfg = config
        if not torch.cuda.is_available() or not ops.device_ok():
            raise RuntimeError("gymrl_amd.ESTrainer needs an MI355X and libgymrl_hip.so; no CPU fallback")
        if ops.ENV_KINDS.get(config.env_name) != ops.LUNARLANDER:
            raise ValueError(f"es_lunarlander.ESTrainer: the evaluator plays LunarLander-v3, not {config.env_name!r}")
        self.device = torch.device(config.device if ":" in str(config.device) else f"cuda:{torch.cuda.current_device()}")
        self.base_seed = 0 if config.seed is None else int(config.seed)
        if config.policy not in POLICIES:
            raise ValueError(f"es_lunarlander.ESTrainer: policy is one of {POLICIES}, not {config.policy!r}")
        self.recurrent = config.policy == "mlprnn"
        state_dim, action_dim, _, _ = ops.env_dims(ops.LUNARLANDER)
        g = torch.random.get_rng_state()
        torch.manual_seed(self.base_seed)
        if self.recurrent:
            from .ppg_rnn_lunarlander import ActorCriticPPG
            self.model = ActorCriticPPG(state_dim, action_dim, hidden_size=64)
        else:
            self.model = ActorCritic(state_dim, action_dim, config.hidden_dim)
        torch.random.set_rng_state(g)
        if self.recurrent:
            named = [n for n, _ in self.model.named_parameters()]
            critic = [n for n in named if n.startswith("critic_fc.")]
            aux = [n for n in named if n.startswith("aux_critic_fc.")]
            trunk = [n for n in named if n not in critic and n not in aux]
            self.flat_params, _ = flatten_module(self.model, self.device, order=critic + trunk + aux)      # PPGTrainer's
            self._act_params = ops.mlprnn_params(self.model)       # the centre in place: views of flat_params
        else:
            self.flat_params, _ = flatten_module(self.model, self.device, order=ppo_net.LAYOUT)
            if not self.model._act_net():
                raise ValueError(f"es_lunarlander.ESTrainer: the one-launch forward takes no hidden width {config.hidden_dim} "
                                 "(include/gymrl.h)")
        self.es = make_learner(config, self.flat_params, self.base_seed)
        self.stack = None                    # the population in the evaluator's layout: one object for the run
        self.last_returns = None             # f64[P, E] on the device: what the last generation's launch returned
        self.history = []                    # (generation, mean population return) at the logged generations

    @property
    def generation(self):
        return self.es.generation

    def train_stream_id0(self, generation=None):
        g = self.es.generation if generation is None else generation
        return self.TRAIN_ENV_ID0 + g * self.cfg.episodes_per_policy

    @torch.no_grad()
    def step_generation(self):
        """ask -> pack ("mlp" only) -> the evaluator's launch -> tell; nothing read back, nothing allocated for the stack after
        the first generation."""
        params = self.es.ask()
        seed, E = self.base_seed + self.EVAL_SEED_OFFSET, self.cfg.episodes_per_policy
        if self.recurrent:
            if self.stack is None or self.stack.buffer is not params:
                self.stack = ops.MlprnnPolicyStack(self.model, self.flat_params, params, copy=False)
            returns = ops.lunar_mlprnn_eval(self.stack, E, seed, self.train_stream_id0(), want_terminal_obs=False)[0]
        else:
            self.stack = ops.LunarPolicyStack(self.model._act_net(), self.flat_params, params, out=self.stack)
            returns = ops.lunar_policy_eval(self.stack, E, seed, self.train_stream_id0(), want_terminal_obs=False)[0]
        self.es.tell(returns if self.cfg.method == "snes" else returns.to(torch.float32))
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

    def _centre_net(self):
        net = self.model._act_net()
        net.refresh()                        # packs the centre as it is now
        return net

    @torch.no_grad()
    def evaluate(self, num_episodes, params=None, stream_offset=0):
        """PPOTrainer.evaluate: -> (returns f64, lengths i32, terminated u8), numpy arrays [P, num_episodes], whole deterministic
        episodes on eval()'s streams (env id (1 << 40) + stream_offset + e) in ONE launch.  params = None: the centre (P = 1);
        params = f32[P, n]: a stack of flat parameter vectors in the layout of flat_params.  Moves nothing of the learner's."""
        if params is not None:
            params = torch.as_tensor(params, dtype=torch.float32).to(self.device)
            params = params.view(1, -1) if params.dim() == 1 else params
        seed, id0 = self.base_seed + self.EVAL_SEED_OFFSET, self.EVAL_ENV_ID0 + int(stream_offset)
        if self.recurrent:
            policy = self._act_params
            if params is not None:
                policy = ops.MlprnnPolicyStack(self.model, self.flat_params, params[:, :self.flat_params.numel()])
            out = ops.lunar_mlprnn_eval(policy, int(num_episodes), seed, id0, want_terminal_obs=False)
        else:
            policy = self._centre_net()
            if params is not None:
                policy = ops.LunarPolicyStack(policy, self.flat_params, params)
            out = ops.lunar_policy_eval(policy, int(num_episodes), seed, id0, want_terminal_obs=False, device=self.device)
        return tuple(t.cpu().numpy() for t in out[:3])

    @torch.no_grad()
    def eval(self, num_episodes=10):
        """The centre's returns over num_episodes deterministic episodes, ONE launch on eval()'s streams (env ids from 1 << 40)
        -> a list of floats, the float32 casts PPOTrainer.eval() lists under fused_eval."""
        seed = self.base_seed + self.EVAL_SEED_OFFSET
        if self.recurrent:
            returns = ops.lunar_mlprnn_eval(self._act_params, int(num_episodes), seed, self.EVAL_ENV_ID0, want_terminal_obs=False)[0]
        else:
            returns = ops.lunar_policy_eval(self._centre_net(), int(num_episodes), seed, self.EVAL_ENV_ID0, want_terminal_obs=False,
                                            device=self.device)[0]
        return returns[0].to(torch.float32).tolist()

    def test(self):
        returns = self.eval(num_episodes=5)
        print(f"test: mean return {sum(returns) / len(returns):.2f} over {len(returns)} episodes")
        return returns

    def save_checkpoint(self, path):
        """The actor-critic under ppo_lunarlander's key (`model_state_dict`): a PPOTrainer of the same hidden width loads an
        ES-found policy with load_checkpoint() and finds no optimiser state.  The recurrent network goes under `es_net_state_dict`,
        a key no other trainer reads: it was found on raw observations and PPGTrainer normalises."""
        from .utils import checkpoint
        return checkpoint.save_agent(path, {self._net_key(): self.model}, {}, es_state_dict=self.es.state_dict(),
                                     generation=self.es.generation, history=list(self.history), method=self.cfg.method,
                                     policy=self.cfg.policy)

    def _net_key(self):
        return "es_net" if self.recurrent else "model"

    def load_checkpoint(self, path):
        from .utils import checkpoint
        check_policy(torch.load(path, map_location="cpu", weights_only=False), self.cfg.policy)       # before a key is missed
        rest = checkpoint.load_agent(path, {self._net_key(): self.model}, {})
        check_method(rest, self.cfg.method)
        self.es.load_state_dict(rest["es_state_dict"])
        self.history = [tuple(h) for h in rest.get("history", [])]
        return rest


if __name__ == "__main__":       # python -m gymrl_amd.es_lunarlander [--<Config attribute> <value> ...]
    from .utils.cli import run_script
    run_script(Config, ESTrainer)

"""OpenAI-ES on a flat parameter buffer (csrc/es.hip): mirrored sampling, centred-rank fitness shaping, Adam on the
search gradient.  No reference script stands behind it; the learner is what the one-launch population evaluators
(policy_eval.PolicyEval.evaluate, ppo_lunarlander.evaluate) were built to feed.

    stack = es.ask()                      # f32[P, stride]: rows 2k / 2k + 1 = theta +- sigma * eps_k          (one launch)
    returns = <any evaluator>(params=stack)  # f32[P, E] on the device                                         (the caller's)
    es.tell(returns)                      # ranks + search gradient, then Adam on theta   (two launches; three above 256 policies)

The perturbations come from the library's counter RNG keyed (seed, generation, pair, element): they are drawn in registers by
both kernels and never stored, and a run replays or resumes bit for bit from (theta, Adam's moments, generation, sigma, seed).
The learner knows nothing about environments or layer layouts."""
import torch

from . import ops
from .flat import FusedAdam


class OpenAIES:
    def __init__(self, flat_params, seed, population, sigma, lr, betas=(0.9, 0.999), eps=1e-8):
        if flat_params.dim() != 1 or flat_params.dtype != torch.float32:
            raise ValueError("OpenAIES: flat_params is a flat float32 buffer")
        if population < 2 or population % 2 or population > ops.ES_MAX_POPULATION:
            raise ValueError(f"OpenAIES: the population is mirrored pairs, an even count in 2..{ops.ES_MAX_POPULATION}")
        if not sigma > 0.0:
            raise ValueError("OpenAIES: sigma > 0")
        self.theta, self.seed, self.population, self.sigma = flat_params, int(seed), int(population), float(sigma)
        n, dev = flat_params.numel(), flat_params.device
        self.stack = torch.zeros(self.population, ops.es_stride(n), dtype=torch.float32, device=dev)
        self.grad = torch.zeros(n, dtype=torch.float32, device=dev)
        self.weights = torch.zeros(self.population, dtype=torch.float32, device=dev)
        self.optimizer = FusedAdam(flat_params, self.grad, lr=lr, betas=betas, eps=eps)      # no clamp, no norm clip
        self.generation = 0

    def ask(self):
        """-> the population of this generation, f32[P, stride] (the learner's own buffer, rewritten by the next ask())."""
        return ops.es_perturb(self.theta, self.sigma, self.seed, self.generation, self.stack)

    def tell(self, returns):
        """returns f32[P, E] on the device, row p the episodes of ask()'s row p: one Adam step of the centre up the shaped
        fitness, and the generation counter moves on.  Nothing is read back."""
        if tuple(returns.shape[:1]) != (self.population,):
            raise ValueError(f"OpenAIES.tell: {self.population} policies were asked, returns is {tuple(returns.shape)}")
        ops.es_shape_grad(returns, self.sigma, self.seed, self.generation, self.grad, self.weights)
        self.optimizer.step()
        self.generation += 1

    def state_dict(self):
        """Adam's moments and step, the generation, sigma and seed — and the centre itself: a flat buffer's alignment gaps are
        perturbed and stepped like any other element, and a module's state_dict() does not carry them."""
        opt = self.optimizer
        return dict(theta=self.theta.detach().cpu().clone(), m=opt.m.detach().cpu().clone(), v=opt.v.detach().cpu().clone(),
                    step=opt.step_count, param_groups=[dict(opt.param_groups[0])], generation=self.generation, sigma=self.sigma,
                    seed=self.seed)

    def load_state_dict(self, sd):
        self.theta.copy_(sd["theta"].to(self.theta.device))
        self.optimizer.load_state_dict(sd)
        self.generation, self.sigma, self.seed = int(sd["generation"]), float(sd["sigma"]), int(sd["seed"])

"""OpenAI-ES on a flat parameter buffer (csrc/es.hip): mirrored sampling, centred-rank fitness shaping, Adam on the
search gradient.  No reference script stands behind it; the learner is what the one-launch population evaluators
(policy_eval.PolicyEval.evaluate, ppo_lunarlander.evaluate) were built to feed.

    stack = es.ask()                      # f32[P, stride]: rows 2k / 2k + 1 = theta +- sigma * eps_k          (one launch)
    returns = <any evaluator>(params=stack)  # f32[P, E] on the device                                         (the caller's)
    es.tell(returns)                      # ranks + search gradient, then Adam on theta   (two launches; three above 256 policies)

The perturbations come from the library's counter RNG keyed (seed, generation, pair, element): they are drawn in registers by
both kernels and never stored, and a run replays or resumes bit for bit from (theta, Adam's moments, generation, sigma, seed).
The learner knows nothing about environments or layer layouts.

SeparableNES (below) has the same surface and noise, a step size per element and no optimiser launch."""
import math

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


class SeparableNES:
    """Separable NES (Schaul, Glasmachers, Schmidhuber 2011; Wierstra et al. 2014, section 3.5) on a flat parameter buffer
    (csrc/es.hip): OpenAIES's surface, noise, mirrored sampling and centred ranks, with a step size per element that
    the same launch adapts — no hand-set scalar for a buffer that mixes layers, biases and alignment gaps, and no optimiser.

        stack = nes.ask()                     # f32[P, stride]: rows 2k / 2k + 1 = mu +- sigma * eps_k                (one launch)
        returns = <any evaluator>(params=stack)  # [P, E] on the device, float32 or float64, read as it is
        nes.tell(returns)                     # ranks, both moment sums, mu and sigma in place      (one launch; two above 256 policies)

    A run replays or resumes bit for bit from (mu, sigma, generation, seed, the learning rates and the bounds)."""

    def __init__(self, flat_params, seed, population, sigma, eta_mu=1.0, eta_sigma=None, sigma_min=1e-5, sigma_max=None):
        if flat_params.dim() != 1 or flat_params.dtype != torch.float32:
            raise ValueError("SeparableNES: flat_params is a flat float32 buffer")
        if population < 2 or population % 2 or population > ops.ES_MAX_POPULATION:
            raise ValueError(f"SeparableNES: the population is mirrored pairs, an even count in 2..{ops.ES_MAX_POPULATION}")
        if not sigma > 0.0:
            raise ValueError("SeparableNES: sigma > 0")
        if not flat_params.is_cuda:
            raise RuntimeError("SeparableNES: flat_params lives on the MI355X; there is no CPU fallback")
        n, dev = flat_params.numel(), flat_params.device
        self.mu, self.seed, self.population = flat_params, int(seed), int(population)
        self.eta_mu = float(eta_mu)
        self.eta_sigma = (3.0 + math.log(n)) / (5.0 * math.sqrt(n)) if eta_sigma is None else float(eta_sigma)
        self.sigma_min, self.sigma_max = float(sigma_min), 10.0 * float(sigma) if sigma_max is None else float(sigma_max)
        if not 0.0 < self.sigma_min <= self.sigma_max:
            raise ValueError("SeparableNES: 0 < sigma_min <= sigma_max")
        self.sigma = torch.full((n,), float(sigma), dtype=torch.float32, device=dev)
        self.stack = torch.zeros(self.population, ops.es_stride(n), dtype=torch.float32, device=dev)
        self.weights = torch.zeros(self.population, dtype=torch.float32, device=dev)
        self.generation = 0

    def ask(self):
        """-> the population of this generation, f32[P, stride] (the learner's own buffer, rewritten by the next ask())."""
        return ops.snes_perturb(self.mu, self.sigma, self.seed, self.generation, self.stack)

    def tell(self, returns):
        """returns [P, E] on the device (float32 or float64), row p the episodes of ask()'s row p: the centre moves up the shaped
        fitness, every step size grows or shrinks, and the generation counter moves on.  Nothing is read back."""
        if tuple(returns.shape[:1]) != (self.population,):
            raise ValueError(f"SeparableNES.tell: {self.population} policies were asked, returns is {tuple(returns.shape)}")
        ops.snes_tell(returns, self.mu, self.sigma, self.seed, self.generation, self.eta_mu, self.eta_sigma, self.sigma_min,
                      self.sigma_max, self.weights)
        self.generation += 1

    def state_dict(self):
        """The centre and the step sizes (alignment gaps included: a module's state_dict() does not carry them), the generation,
        the seed, the learning rates and the bounds."""
        return dict(mu=self.mu.detach().cpu().clone(), sigma=self.sigma.detach().cpu().clone(), generation=self.generation,
                    seed=self.seed, eta_mu=self.eta_mu, eta_sigma=self.eta_sigma, sigma_min=self.sigma_min,
                    sigma_max=self.sigma_max)

    def load_state_dict(self, sd):
        self.mu.copy_(sd["mu"].to(self.mu.device))
        self.sigma.copy_(sd["sigma"].to(self.sigma.device))
        self.generation, self.seed = int(sd["generation"]), int(sd["seed"])
        self.eta_mu, self.eta_sigma = float(sd["eta_mu"]), float(sd["eta_sigma"])
        self.sigma_min, self.sigma_max = float(sd["sigma_min"]), float(sd["sigma_max"])

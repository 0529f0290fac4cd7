"""Hand-scheduled forward / loss / backward of the PPO ActorCritic for the update phase — ONE path:
`FusedActorCriticUpdate.step()`.  Every contraction is a hand-written exact-f32 MFMA kernel of csrc/gemm.hip (hidden
widths 64 / 128 / 256) and every elementwise / reduction pass an HBM-bound kernel of csrc/mlp_train.hip; autograd and
the GEMM libraries are not on this path.

    forward   H1  = tanh(X W1^T + b1)                 gymrl_linear_tanh_smallk   (K = obs_dim)
              H2  = tanh(H1 W2^T + b2)                gymrl_linear_fwd, tanh in the MFMA epilogue
              Zac = H2 [Wa1;Wc1]^T + [ba1;bc1]        gymrl_linear_fwd (N = 2 hidden, bias only: the heads pass applies
                                                      the tanh where the VALU is idle)
    loss+heads  dZac (in place), dbac, dWa2, dba2, dWc2, dbc2, metrics
                                                      hidden 256, and three actions at every width:
                                                      gymrl_heads_loss_fwd_bwd, ONE pass over Zac;
                                                      hidden 64 / 128 with 2 or 4 actions: gymrl_heads_fwd_tanh ->
                                                      gymrl_ppo_loss_fwd_bwd -> gymrl_heads_bwd (the same per-row
                                                      arithmetic as three passes; gymrl_heads_bwd takes no A = 3);
                                                      FusedGaussianUpdate (the Gaussian head, one mean): always
                                                      gymrl_gauss_heads_loss_fwd_bwd, ONE pass that also writes dlog_std
    backward  d[Wa1;Wc1] = dZac^T H2                  gymrl_linear_bwd_weight (hidden 256) / gymrl_lin_bwd_weight
              dZ2 = (dZac [Wa1;Wc1]) (1 - H2^2)       gymrl_linear_bwd_input, tanh' in the epilogue
              dW2 = dZ2^T H1, db2 = colsum dZ2        gymrl_linear_bwd_weight / gymrl_lin_bwd_weight (+ bias gradient)
              dZ1 = (dZ2 W2) (1 - H1^2)               gymrl_linear_bwd_input
              dW1 = dZ1^T X, db1 = colsum dZ1         gymrl_linear_smallk_bwd (dZ given)

`ActorCritic.evaluate_actions` + `loss.backward()` (ppo_lunarlander.py:110-117, :303) on a B = 262,144-row minibatch is,
under autograd, 10 library GEMMs plus ~30 elementwise / reduction launches that each stream a [B, 256] activation
through HBM.  (The round-1 schedule — library GEMMs + separate passes — lives in tools/legacy_update_path.py as the A/B
baseline of tools/micro_update.py.)

The parameters stay the module's own nn.Parameters (state_dict-compatible with the reference);
`flatten_module(order=LAYOUT)` only places actor.0 / critic.0 next to each other in the flat
buffer so that [Wa1;Wc1] and [ba1;bc1] are plain views.  Gradients are written (not
accumulated) into the parameters' .grad views of the flat gradient buffer.
"""
import torch

from . import ops

# flat-buffer order that makes [actor.0 ; critic.0] contiguous (weights, then biases)
LAYOUT = ["shared.0.weight", "shared.0.bias", "shared.2.weight", "shared.2.bias",
          "actor.0.weight", "critic.0.weight", "actor.0.bias", "critic.0.bias",
          "actor.2.weight", "actor.2.bias", "critic.2.weight", "critic.2.bias"]


def supported(model):
    H = model.shared[0].out_features
    D = model.shared[0].in_features
    A = model.actor[2].out_features
    # H in {64, 128, 256}, D in {2, 3, 4, 6, 8}, A in {2, 3, 4}: the library states the gate (gymrl_ppo_update_shape_ok).
    # multiples of 64 keep flatten_module's 64-float padding from separating actor.0 / critic.0
    return (ops.ppo_update_shape_ok(H, D, A)
            and model.shared[2].out_features == H and model.actor[0].out_features == H
            and model.critic[0].out_features == H)


def gauss_supported(model):
    """supported() for the Gaussian head (ppo_pendulum.GaussianActorCritic): the library's own gate
    (gymrl_ppo_gauss_update_shape_ok: H in {64, 128, 256}, D in {2, 3, 4, 6, 8}, A == 1), the same widths, and a log_std."""
    H = model.shared[0].out_features
    D = model.shared[0].in_features
    A = model.actor[2].out_features
    return (ops.ppo_gauss_update_shape_ok(H, D, A)
            and model.shared[2].out_features == H and model.actor[0].out_features == H
            and model.critic[0].out_features == H and hasattr(model, "log_std"))


class FusedActorCriticUpdate:
    _covers = staticmethod(supported)      # the shapes this schedule takes (FusedGaussianUpdate: gauss_supported)

    def __init__(self, model, max_rows):
        if not self._covers(model):
            raise ValueError("unsupported ActorCritic shape for the fused update path")
        self.m = model
        W1 = model.shared[0].weight
        dev = W1.device
        self.H, self.D, self.A = W1.shape[0], W1.shape[1], model.actor[2].out_features
        H = self.H
        wa, wc = model.actor[0].weight, model.critic[0].weight
        ba, bc = model.actor[0].bias, model.critic[0].bias
        if wc.data_ptr() != wa.data_ptr() + wa.numel() * 4 or bc.data_ptr() != ba.data_ptr() + ba.numel() * 4:
            raise ValueError("actor.0 / critic.0 are not adjacent: flatten_module(model, device, order=ppo_net.LAYOUT)")
        flat, gflat = model._flat_params, model._flat_grads

        def view(p, n, shape, buf):
            off = (p.data_ptr() - flat.data_ptr()) // 4
            return buf[off:off + n].view(shape)
        self.Wac = view(wa, 2 * H * H, (2 * H, H), flat)
        self.bac = view(ba, 2 * H, (2 * H,), flat)
        self.dWac = view(wa, 2 * H * H, (2 * H, H), gflat)
        self.dbac = view(ba, 2 * H, (2 * H,), gflat)
        self.ws = ops.mlp_train_workspace(H, self.D, self.A, dev)
        R = int(max_rows)
        self.R = R
        self.H1 = torch.empty(R, H, device=dev)
        self.H2 = torch.empty(R, H, device=dev)
        self.Hac = torch.empty(R, 2 * H, device=dev)
        self.dH2 = torch.empty(R, H, device=dev)
        self.dH1 = torch.empty(R, H, device=dev)
        self.timers = None      # bench.py: KernelTimers bracketing every launch
        # two independent choices.  The heads: gymrl_heads_loss_fwd_bwd (one pass) at hidden 256 and wherever A = 3, which
        # gymrl_heads_bwd does not take.  The weight gradients: the 256-deep GEMM (gemm_ws) at hidden 256, the narrow
        # kernels of lin.hip (lin_ws) below it.
        self.one_pass_heads, defer = self._schedule()
        self.gemm_ws = ops.gemm_workspace(dev) if H == 256 else None
        # the five batch reductions' second halves as ONE launch at the end of step() (gymrl_update_finalize) instead of five
        # behind their producers: every producer then keeps its partials in a workspace of its own until that launch
        self.defer_finalize = defer
        self.gemm_ws2 = ops.gemm_workspace(dev) if defer else None
        self.ws2 = ops.mlp_train_workspace(H, self.D, self.A, dev) if defer else None
        if not self.one_pass_heads:
            self.logits = torch.empty(R, self.A, device=dev)
            self.value = torch.empty(R, 1, device=dev)
            self.dlogits = torch.empty(R, self.A, device=dev)
            self.dvalue = torch.empty(R, device=dev)
        if H != 256:
            self.lin_ws = ops.lin_workspace(R, 2 * H, H, 1, dev) if R > 512 else None

    def _schedule(self):
        """(one-pass heads, deferred finalize) for this shape."""
        return self.H == 256 or self.A == 3, self.H == 256

    def _heads_one_pass(self, t, sfx, B, Zac, heads, act, logp_old, adv, ret, loss_cfg, adv_moments, dbac, hg, metric_parts):
        """The one pass over Zac: loss, dZac in place, the heads' gradients (or their block partials) and the metric partials."""
        t("heads_loss_fwd_bwd" + sfx, B, ops.heads_loss_fwd_bwd, Zac, None, *heads, act, logp_old, adv, ret, loss_cfg, adv_moments,
          dbac, *hg, metric_parts, self.ws)

    def _timed(self, name, units, fn, *args, **kw):
        tm = self.timers
        if tm is None:
            return fn(*args, **kw)
        tm.start(name)
        r = fn(*args, **kw)
        tm.stop(name, units)
        return r

    def metric_blocks(self, B):
        """Rows of the f64[blocks, 5] metric-partials buffer step() fills for a minibatch of B rows."""
        return ops.heads_loss_blocks(B, self.H) if self.one_pass_heads else ops.loss_blocks(B)

    @torch.no_grad()
    def step(self, x, act, logp_old, adv, ret, loss_cfg, adv_moments, metric_parts, reducer=None):
        """Forward, loss and backward of one minibatch (module docstring): writes every parameter gradient
        (overwrite) and the f64[metric_blocks(B), 5] partial metric sums.  `reducer` (dist.GradReducer with its
        split at actor.0.weight): bucket 1 = [actor.0 | critic.0, heads] is launched as soon as its last writer is
        queued, bucket 0 = the trunk after the last kernel."""
        m, B, H = self.m, x.shape[0], self.H
        if B > self.R:
            raise ValueError("minibatch larger than the buffers")
        t = self._timed
        H1, H2, Zac, dZ2, dZ1 = self.H1[:B], self.H2[:B], self.Hac[:B], self.dH2[:B], self.dH1[:B]
        W2, ws = m.shared[2].weight, self.gemm_ws
        sfx = "" if H == 256 else f"_h{H}"
        t("linear_tanh_smallk", B, ops.linear_tanh_smallk, x, m.shared[0].weight, m.shared[0].bias, H1)
        t(f"gemm_fwd_{H}_tanh", B, ops.linear_fwd, H1, W2, m.shared[2].bias, H2, True)
        t(f"gemm_fwd_{2 * H}", B, ops.linear_fwd, H2, self.Wac, self.bac, Zac, False)
        heads = (m.actor[2].weight, m.actor[2].bias, m.critic[2].weight, m.critic[2].bias)
        hgrads = (m.actor[2].weight.grad, m.actor[2].bias.grad, m.critic[2].weight.grad, m.critic[2].bias.grad)
        # (multi-rank: bucket 1 of the gradient all-reduce leaves in the middle of step(): its gradients are finalized at once)
        wide = H == 256                                   # weight gradients: the 256-deep GEMM / lin.hip's narrow kernels
        defer = self.defer_finalize and self.one_pass_heads and wide and reducer is None
        if self.one_pass_heads:
            dbac, hg = (None, (None,) * 4) if defer else (self.dbac, hgrads)
            self._heads_one_pass(t, sfx, B, Zac, heads, act, logp_old, adv, ret, loss_cfg, adv_moments, dbac, hg, metric_parts)
        else:
            logits, value, dl, dv = self.logits[:B], self.value[:B], self.dlogits[:B], self.dvalue[:B]
            # the GEMM added [ba1;bc1]: the heads read pre-activations, recompute their tanh in backward, write dZac in place
            t("heads_fwd_tanh" + sfx, B, ops.heads_fwd_tanh, Zac, heads[0], heads[1], heads[2], heads[3], logits, value, None, False)
            t("ppo_loss_fwd_bwd" + sfx, B, ops.ppo_loss_fwd_bwd, logits, value.view(-1), act, logp_old, adv, ret, loss_cfg,
              adv_moments=adv_moments, dlogits_out=dl, dvalue_out=dv, workspace=metric_parts)
            t("heads_bwd" + sfx, B, ops.heads_bwd, Zac, dl, dv, heads[0], heads[2], Zac, self.dbac, hgrads[0], hgrads[1],
              hgrads[2], hgrads[3], self.ws, True, None)
        if wide:
            t("gemm_dw_512", B, ops.linear_bwd_weight, Zac, H2, None if defer else self.dWac, ws)
        else:
            t(f"lin_dw_{2 * H}", B, ops.lin_bwd_weight, Zac, None, H2, self.dWac, workspace=self.lin_ws)
        if reducer is not None:
            reducer.launch(1)
        t(f"gemm_dx_{2 * H}_tanhbwd", B, ops.linear_bwd_input, Zac, self.Wac, H2, dZ2)
        if defer:
            t("gemm_dw_256_db", B, ops.linear_bwd_weight, dZ2, H1, None, self.gemm_ws2, None, True)
        elif wide:
            t("gemm_dw_256_db", B, ops.linear_bwd_weight, dZ2, H1, W2.grad, ws, m.shared[2].bias.grad)
        else:
            t(f"lin_dw_{H}_db", B, ops.lin_bwd_weight, dZ2, None, H1, W2.grad, m.shared[2].bias.grad, workspace=self.lin_ws)
        t(f"gemm_dx_{H}_tanhbwd", B, ops.linear_bwd_input, dZ2, W2, H1, dZ1)
        if defer:
            t("linear_smallk_bwd", B, ops.linear_smallk_bwd, dZ1, None, x, None, None, self.ws2)
            t("update_finalize", B, ops.update_finalize, B, H, self.A, self.D, ws, self.dWac, self.gemm_ws2, W2.grad,
              m.shared[2].bias.grad, self.ws, self.dbac, hgrads[0], hgrads[1], hgrads[2], hgrads[3], self.ws2,
              m.shared[0].weight.grad, m.shared[0].bias.grad)
        else:
            t("linear_smallk_bwd", B, ops.linear_smallk_bwd, dZ1, None, x, m.shared[0].weight.grad, m.shared[0].bias.grad,
              self.ws)
        if reducer is not None:
            reducer.launch(0)


class FusedGaussianUpdate(FusedActorCriticUpdate):
    """FusedActorCriticUpdate.step() for ppo_pendulum.GaussianActorCritic: the same launches around the heads, and the heads as
    gymrl_gauss_heads_loss_fwd_bwd — always the one pass, never the deferred finalize (gymrl_update_finalize is the categorical
    head's; hidden 256 takes step()'s non-deferred calls).  `act` arrives as the minibatch's packed int32 column and is read as
    the float32 bits it holds; d(loss) / d(log_std) goes straight into model.log_std.grad's view of the flat gradient."""
    _covers = staticmethod(gauss_supported)

    def __init__(self, model, max_rows):
        super().__init__(model, max_rows)
        self.log_std = model.log_std.detach()          # the parameter's view of the flat buffer
        self.dlog_std = model.log_std.grad             # ... and of the flat gradient
        if self.dlog_std is None or self.dlog_std.untyped_storage().data_ptr() != model._flat_grads.untyped_storage().data_ptr():
            raise ValueError("log_std.grad is not a view of the flat gradient: flatten_module(model, device, order=ppo_net.LAYOUT)")
        self.dls_ws = ops.gauss_heads_loss_workspace(self.R, self.H, self.A, model.shared[0].weight.device)

    def _schedule(self):
        return True, False

    def _heads_one_pass(self, t, sfx, B, Zac, heads, act, logp_old, adv, ret, loss_cfg, adv_moments, dbac, hg, metric_parts):
        t("gauss_heads_loss_fwd_bwd" + sfx, B, ops.gauss_heads_loss_fwd_bwd, Zac, None, *heads, self.log_std,
          act.view(torch.float32).view(-1, self.A), logp_old, adv, ret, loss_cfg, adv_moments, dbac, *hg, self.dlog_std, metric_parts,
          self.ws, self.dls_ws)

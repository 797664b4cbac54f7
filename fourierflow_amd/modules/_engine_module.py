"""What every engine-backed operator module shares: the parameter list handed to the host engine, the one autograd node
around ``engine.forward`` / ``engine.backward`` and the inference path without a node.

A module mixes :class:`EngineModule` in, builds its parameter tree like the reference, provides ``engine()`` and ends its
``forward()`` in ``self._apply_engine(x)``.
"""
import torch


def flat_grads(eng, flat):
    """The engine's flat gradient buffer cut into per-parameter views, in ``param_names`` order."""
    grads, off = [], 0
    for n in eng.param_names:
        shape = eng.param_shapes[n]
        cnt = 1
        for s in shape:
            cnt *= s
        grads.append(flat[off:off + cnt].view(shape))
        off += cnt
    return grads


class _EngineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, module, *params):
        eng = module._engine_for(params)
        y, ctx.token = module._run_forward(eng, x, any(ctx.needs_input_grad))
        ctx.module = module
        return y

    @staticmethod
    def backward(ctx, gy):
        module = ctx.module
        eng = module._engine
        # the reference modules are ordinary autograd modules: dL/dx goes to whatever produced the input (grid_2d.py:154-177)
        flat, dx = module._run_backward(eng, ctx.token, gy.contiguous(), ctx.needs_input_grad[0])
        # (a copy: the engine reuses its gradient buffer)
        grads = [None] * len(eng.param_names) if flat is None else flat_grads(eng, flat.clone())
        return (dx if ctx.needs_input_grad[0] else None, None, *grads)


class EngineModule:
    """Mixin of the ``nn.Module`` mirrors whose arithmetic runs in a host engine (``self.engine()``)."""

    _engine = None          # built by engine() on first use; ``module._engine = None`` drops it
    _generation = 0         # forward passes so far: the activations live in one pre-allocated workspace

    def engine_parameters(self):
        """Unique parameters in the engine's flat-buffer order (reference named_parameters() names)."""
        eng = self.engine()
        slots = self.__dict__.get("_param_slots")
        if slots is None:
            # where each engine parameter lives: (owning submodule, attribute).  The module tree is fixed after construction, so
            # the walk over named_parameters() (0.3 ms of a 0.7 ms batch-1 forward) is done once; the Parameter objects are
            # re-read from their owners on every call (a replaced or re-registered Parameter is seen).
            owners = {}
            for prefix, mod in self.named_modules():
                for attr in mod._parameters:
                    owners.setdefault(prefix + ("." if prefix else "") + attr, (mod, attr))
            slots = [(n,) + owners[n] for n in eng.param_names]
            self.__dict__["_param_slots"] = slots
        return [(n, mod._parameters[attr]) for n, mod, attr in slots]

    def prepare_input(self, x):
        return x

    def _engine_for(self, params):
        eng = self.engine()
        eng.bind({n: p.detach() for n, p in zip(eng.param_names, params)})
        return eng

    def _apply_engine(self, x):
        params = [p for _, p in self.engine_parameters()]
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
            return _EngineFn.apply(x, self, *params)
        # inference: no autograd node (a Function.apply over ~100 tensors costs as much as a third of the kernels)
        return self._run_forward(self._engine_for(params), x, False)[0]

    # -- what the autograd node calls; the defaults serve the FFNOEngine family -----------------------
    def _run_forward(self, eng, x, save):
        """-> (output, token): the token comes back to ``_run_backward``."""
        # (dropout follows nn.Module.training like the reference)
        return eng.forward(x, save, training=self.training), self._new_pass()

    def _new_pass(self):
        self._generation += 1
        return self._generation

    def _check_latest(self, token):
        if self._generation != token:
            raise RuntimeError(f"{type(self).__name__}: only the most recent forward pass can be back-propagated "
                               "(activations live in one pre-allocated workspace)")

    def _run_backward(self, eng, token, gy, need_dx):
        """-> (flat gradient buffer or None, input gradient or None)."""
        self._check_latest(token)
        flat = eng.backward(gy, need_dx=need_dx)
        return flat, eng.dx

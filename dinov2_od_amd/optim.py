"""The optimizer step of the training loop on the HIP kernels of csrc/optim.hip.

    from dinov2_od_amd.optim import Adam, AdamW, ModelEMA, clip_grad_norm_

`Adam` is `torch.optim.Adam` with three more arguments.  `max_grad_norm`: the reference's
`clip_grad_norm_(model.parameters(), gradient_clip_val)` + `optimizer.step()` (train.py:1101-1110) as
one call of two launches -- the gradients' sum of squares, then clip and update fused.
`skip_nonfinite`: a step whose gradient norm is inf or NaN changes nothing (see `Adam`).  `ema`: a
`ModelEMA` whose shadows the update launch writes in the same pass.  `AdamW` is the same over
`torch.optim.AdamW` (decoupled weight decay), and `Adam(..., decoupled_weight_decay=True)` is `AdamW`.
Their state is PyTorch's (`step` CPU tensor, `exp_avg`, `exp_avg_sq`), so `state_dict()` /
`load_state_dict()` interchange with `torch.optim.Adam` / `torch.optim.AdamW` in both directions.

The kernels take contiguous fp32 CUDA parameters with dense contiguous fp32 gradients on one
device, L2 or decoupled weight decay, no amsgrad / maximize / capturable / differentiable / fused /
tensor lr.  Every other configuration PyTorch accepts runs PyTorch's own step (after `clip_grad_norm_`
below when `max_grad_norm` is set): an explicit delegation of the cases the kernels do not implement,
never a substitute for a kernel that is missing -- on the native path a missing library raises.
`skip_nonfinite` exists on the native path only: a step that would be delegated raises instead of
silently not skipping.

The kernels write through `data_ptr()`, which autograd's version counters do not see; the engine
keys its packed weights on `(data_ptr, _version)` (engine.py), so every parameter, every shadow of
the average (and every gradient the standalone clip scales) is bumped with
`torch.autograd.graph.increment_version`.
"""
import copy
import ctypes as C
import math

import numpy as np
import torch

from . import _native

__all__ = ["Adam", "AdamW", "ModelEMA", "clip_grad_norm_"]

_F32, _STRIDED = torch.float32, torch.strided
# struct dod_optim_tensor as a numpy record: the step fills whole columns instead of 7 ctypes fields per tensor
_DESC = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i8"), ("step_size", "<f4"), ("bc2_sqrt", "<f4")])
assert _DESC.itemsize == C.sizeof(_native.DodOptimTensor)
_EMA_DESC = np.dtype([("e", "<u8"), ("p", "<u8"), ("n", "<i8")])       # struct dod_optim_ema_tensor
assert _EMA_DESC.itemsize == C.sizeof(_native.DodOptimEmaTensor)
_check = _native.check


def _dense_f32_cuda(t):
    return t.is_cuda and t.dtype == torch.float32 and t.layout == torch.strided and t.is_contiguous()


def _workspace(n_tensors, total, device):
    nbytes = _native.lib().dod_optim_workspace_bytes(n_tensors, total)
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """torch.nn.utils.clip_grad_norm_ (same signature, same 0-dim device tensor returned) in two launches for the 2-norm of
    dense fp32 CUDA gradients on one device; every other case is PyTorch's."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    parameters = list(parameters)
    grads = [p.grad for p in parameters if p.grad is not None]
    native = bool(grads) and float(norm_type) == 2.0 and not error_if_nonfinite and all(_dense_f32_cuda(g) for g in grads) \
        and len({g.device for g in grads}) == 1
    if not native:
        return torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type, error_if_nonfinite, foreach)
    dev = grads[0].device
    arr = (_native.DodOptimTensor * len(grads))()
    total = 0
    for d, g in zip(arr, grads):
        d.g, d.n = g.data_ptr(), g.numel()
        total += d.n
    with torch.cuda.device(dev):
        norm = torch.empty((), dtype=torch.float32, device=dev)
        ws, nbytes = _workspace(len(grads), total, dev)
        _check(_native.lib().dod_optim_clip_grad_norm(arr, len(grads), float(max_norm), _native.ptr(norm), _native.ptr(ws), nbytes,
                                                      _native.stream_ptr()))
    torch.autograd.graph.increment_version(grads)
    return norm


class _Pairs:
    """e += (p - e) w over [(shadow, parameter)]: one launch of the standalone kernel per device for dense fp32 CUDA pairs, the same
    formula in torch float64 (two rounded double operations, one rounding to the shadow's type) for every other pair -- the same bits.
    The checks and the descriptors are made once, and again when a tensor's data pointer moved (.to(), .half(), an assigned load)."""

    def __init__(self, pairs):
        self.pairs = list(pairs)
        self.shadows = [e for e, _ in self.pairs]
        self.ptrs = None

    def _prepare(self, ptrs):
        by_dev, self.rest = {}, []
        for e, p in self.pairs:
            if _dense_f32_cuda(e) and _dense_f32_cuda(p) and e.device == p.device and e.shape == p.shape:
                by_dev.setdefault(e.device, []).append((e, p))
            else:
                self.rest.append((e, p))
        self.native = []
        for dev, lst in by_dev.items():
            d = np.empty(len(lst), dtype=_EMA_DESC)
            d["e"] = [e.data_ptr() for e, _ in lst]
            d["p"] = [p.data_ptr() for _, p in lst]
            d["n"] = [e.numel() for e, _ in lst]
            self.native.append((dev, d))
        self.ptrs = ptrs

    def run(self, w):
        if not self.pairs:
            return
        ptrs = [t.data_ptr() for pair in self.pairs for t in pair]
        if ptrs != self.ptrs:
            self._prepare(ptrs)
        for dev, d in self.native:
            with torch.cuda.device(dev):
                _check(_native.lib().dod_optim_ema_update(d.ctypes.data, len(d), float(w), _native.stream_ptr()))
        if self.rest:
            with torch.no_grad():
                for e, p in self.rest:
                    e64 = e.detach().double()
                    e.copy_(e64 + (p.detach().to(device=e.device, dtype=torch.float64) - e64) * w)
        torch.autograd.graph.increment_version(self.shadows)


class ModelEMA:
    """Exponential moving average of a model's trainable parameters: `e += (p - e)(1 - d)`, `d = decay (1 - exp(-updates / tau))`
    (`tau == 0`: `d = decay`), formed in Python doubles and evaluated in double, rounded once (csrc/optim.hip; torch float64 for
    tensors the kernels do not take, with the same bits).

    `.module` is a copy of `model` in eval() mode that SHARES every parameter with `requires_grad == False` (the frozen backbone: same
    storage, `data_ptr()` equal) and owns fp32 shadows of the trainable ones; buffers are copied as `copy.deepcopy` copies them.
    Evaluate, `detect` and save with `.module`.  `update()` advances `updates`, launches the average over all shadows and bumps their
    version counters, so the module's engine re-packs at its next forward and not before.  Passed as `ema=` to `optim.Adam` / `AdamW`,
    the optimizer's `step()` does all of that inside its update launch; calling `update()` as well then raises.
    `state_dict()` carries `updates`, `decay`, `tau` and the shadows by parameter name."""

    def __init__(self, model, decay=0.9999, tau=0):
        if not 0.0 <= float(decay) <= 1.0 or float(tau) < 0:
            raise ValueError(f"decay = {decay} outside [0, 1] or tau = {tau} negative")
        self.decay, self.tau, self.updates = float(decay), float(tau), 0
        memo = {id(p): p for p in model.parameters() if not p.requires_grad}       # the copy keeps these very objects
        self.module = copy.deepcopy(model, memo)
        self.module.eval()
        shadows = dict(self.module.named_parameters())
        self._names, self._pairs = [], []                   # [(shadow, parameter)], the model's trainable parameters in named order
        for name, p in model.named_parameters():
            if not p.requires_grad:
                continue
            e = shadows[name]
            if e.dtype != _F32:
                e.data = e.data.float()
            e.requires_grad_(False)
            self._names.append(name)
            self._pairs.append((e, p))
        self._model = model
        self._all = _Pairs(self._pairs)
        self._shadow_of = {id(p): e for e, p in self._pairs}
        self._owner = None                                  # the optimizer that drives this average

    def weight(self, updates=None):
        """w = 1 - d of update number `updates` (default: the next one)"""
        k = self.updates + 1 if updates is None else updates
        d = self.decay * (1.0 - math.exp(-k / self.tau)) if self.tau > 0 else self.decay
        return 1.0 - d

    def shadow_of(self):
        """{id(parameter): shadow} for the trainable parameters of the model this average follows"""
        return self._shadow_of

    def _advance(self):
        self.updates += 1
        return self.weight(self.updates)

    def update(self, model=None):
        if self._owner is not None:
            raise RuntimeError("this ModelEMA was passed as ema= to an optimizer, whose step() updates it: do not call update() as well")
        todo = self._all
        if model is not None and model is not self._model:
            theirs = dict(model.named_parameters())
            todo = _Pairs([(e, theirs[n]) for n, (e, _) in zip(self._names, self._pairs)])
        todo.run(self._advance())

    def state_dict(self):
        return {"updates": self.updates, "decay": self.decay, "tau": self.tau,
                "shadows": {n: e.detach().clone() for n, (e, _) in zip(self._names, self._pairs)}}

    def load_state_dict(self, state):
        missing = [n for n in self._names if n not in state["shadows"]]
        if missing or len(state["shadows"]) != len(self._names):
            raise KeyError(f"shadows do not match the model's trainable parameters (missing {missing[:3]})")
        self.updates, self.decay, self.tau = int(state["updates"]), float(state["decay"]), float(state["tau"])
        with torch.no_grad():
            for n, (e, _) in zip(self._names, self._pairs):
                e.copy_(state["shadows"][n])                # copy_ bumps the version counter: the engine re-packs


class Adam(torch.optim.Adam):
    """torch.optim.Adam(...) plus `max_grad_norm` (None = no clipping), `skip_nonfinite` and `ema`.
    `last_grad_norm`: the total gradient norm of the last step as a 0-dim device tensor (no synchronisation), None before the first
    step that formed one.

    `skip_nonfinite=True`: the norm is formed every step (also without clipping), and when it is inf or NaN the update launch returns
    before any store: parameters, both moments and the average keep their bits, and `skipped_steps` (a 0-dim int32 device tensor, never
    synchronised by this class) grows by one.  The host cannot know without a synchronisation, so the CPU `step` tensors (and an
    attached average's `updates`) advance on a skipped step too: `step` counts calls.  After k skips the bias corrections run k steps
    ahead: the update is scaled by `(1 - beta1^t) / (1 - beta1^(t+k)) * sqrt((1 - beta2^(t+k)) / (1 - beta2^t))`, to first order
    `1 - k beta1^t (1 - beta1) / (1 - beta1^t) + k beta2^t (1 - beta2) / (2 (1 - beta2^t))`.  With betas (0.9, 0.999) one skip before
    step 10 changes the 10th update by -5.4 % + 5 % (the two corrections nearly cancel while t << 1/(1 - beta1)), at step 100 by
    +0.5 %, at step 1 000 by +2.9e-4, and the effect dies out as beta2^t.  Tensors whose gradient is None are averaged by a launch
    of their own that does not see the norm.  A step the kernels do not take (see the module docstring) raises RuntimeError with
    this option set.

    `ema=ModelEMA(model)`: the update launch also writes the shadows of the parameters it updates (one more read and write of the
    thread that holds p'); trainable parameters without a gradient go through the standalone kernel in the same `step()`.  On the
    delegated path the average runs after PyTorch's step.  Pickling drops the link to the average."""

    def __init__(self, *args, max_grad_norm=None, skip_nonfinite=False, ema=None, **kwargs):
        super().__init__(*args, **kwargs)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.last_grad_norm = None
        self.skipped_steps = None
        if self.skip_nonfinite:
            dev = self.param_groups[0]["params"][0].device
            if dev.type == "cuda":
                self.skipped_steps = torch.zeros((), dtype=torch.int32, device=dev)
        self.ema = ema
        if ema is not None:
            if ema._owner is not None:
                raise RuntimeError("this ModelEMA already belongs to an optimizer")
            ema._owner = self
        # parameter -> (state dict, exp_avg, exp_avg_sq, step, numpy view of step, pointers of both moments, numel): the state is checked
        # once and again only when one of these objects has been replaced; the parameter and its fresh gradient are checked every step
        self._seen = {}
        self._ws = None
        self._ema_plans = {}
        self._options = _native.DodOptimOptions()

    def __getstate__(self):             # pickled / deep-copied: Optimizer keeps defaults, state and param_groups only
        state = super().__getstate__()
        state["max_grad_norm"] = self.max_grad_norm
        state["skip_nonfinite"] = self.skip_nonfinite
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("max_grad_norm", None)
        self.__dict__.setdefault("skip_nonfinite", False)
        self.__dict__.setdefault("last_grad_norm", None)
        self.__dict__.setdefault("skipped_steps", None)
        self.__dict__.setdefault("ema", None)
        self._seen, self._ws, self._ema_plans, self._options = {}, None, {}, _native.DodOptimOptions()

    # ------------------------------------------------------------------ which path
    def _admit(self, p, st):
        """full check of one parameter and its state (created as PyTorch's Adam._init_group creates it); None = not for the kernels"""
        if not _dense_f32_cuda(p):
            return None
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        step, m, v = st.get("step"), st.get("exp_avg"), st.get("exp_avg_sq")
        if not (torch.is_tensor(step) and step.device.type == "cpu" and step.dtype == _F32 and step.dim() == 0):
            return None
        if not all(torch.is_tensor(x) and _dense_f32_cuda(x) and x.device == p.device and x.shape == p.shape for x in (m, v)):
            return None
        seen = self._seen[p] = (st, m, v, step, step.numpy(), m.data_ptr(), v.data_ptr(), p.numel())
        return seen

    def _native_plan(self):
        """what the kernels need for this step, or None when PyTorch's step has to run: (device, [(key, params, grads, seen, lr, decay)])
        with key = (beta1, beta2, eps, L2 weight_decay, decoupled) and decay = 1 - lr * weight_decay of a decoupled group (1.0 otherwise),
        one entry per param group that has gradients"""
        if getattr(self, "grad_scale", None) is not None or getattr(self, "found_inf", None) is not None:
            return None
        plan, device, state, seen_of = [], None, self.state, self._seen
        for group in self.param_groups:
            if group["amsgrad"] or group["maximize"] or group["capturable"] or group["differentiable"] or group["fused"]:
                return None
            lr, (beta1, beta2), eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
            if not all(isinstance(x, (int, float)) for x in (lr, beta1, beta2, eps, wd)):
                return None
            decoupled = bool(group.get("decoupled_weight_decay", False))
            ps, gs, ss = [], [], []
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if device is None:
                    device = p.device
                if not (g.dtype is _F32 and g.layout is _STRIDED and g.is_contiguous() and g.device == device and p.device == device
                        and p.dtype is _F32 and p.is_contiguous()):
                    return None
                st = state[p]
                seen = seen_of.get(p)
                if seen is None or seen[0] is not st or st.get("exp_avg") is not seen[1] or st.get("exp_avg_sq") is not seen[2] \
                        or st.get("step") is not seen[3]:
                    seen = self._admit(p, st)
                    if seen is None:
                        return None
                ps.append(p)
                gs.append(g)
                ss.append(seen)
            if ps:
                key = (float(beta1), float(beta2), float(eps), 0.0 if decoupled else float(wd), decoupled)
                plan.append((key, ps, gs, ss, float(lr), 1 - lr * wd if decoupled else 1.0))      # PyTorch: param.mul_(1 - lr * weight_decay)
        return (device, plan) if plan and device.type == "cuda" else None

    # ------------------------------------------------------------------ the step
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        plan = self._native_plan()
        if plan is None:
            if self.skip_nonfinite:
                raise RuntimeError("skip_nonfinite exists on the native path only (dense fp32 CUDA parameters and gradients on one device, "
                                   "no amsgrad / maximize / capturable / differentiable / fused): this step would run PyTorch's, which does not skip")
            if self.max_grad_norm is not None and self.max_grad_norm > 0:
                self.last_grad_norm = clip_grad_norm_([p for g in self.param_groups for p in g["params"]], self.max_grad_norm)
            base = torch.optim.Adam.step
            if getattr(base, "hooked", False):      # this class's step already runs the step hooks
                base = base.__wrapped__
            base(self)
            if self.ema is not None:
                self.ema._all.run(self.ema._advance())
            return loss
        self._native_step(*plan)
        return loss

    def _native_step(self, dev, plan):
        lib = _native.lib()
        # one call per distinct (betas, eps, L2 weight_decay, decoupled); lr lives in the per-tensor step size and the decoupled decay in a
        # per-tensor factor, so groups that differ in lr (and, decoupled, in weight_decay) alone share a call
        calls = {}
        for key, ps, gs, ss, lr, decay in plan:
            beta1, beta2 = key[0], key[1]
            c = calls.setdefault(key, ([], [], [], [], [], [], [], []))
            bias = {}
            for seen in ss:
                view = seen[4]
                view += 1                           # the CPU `step` tensor, through its numpy view
                t = float(view)
                if t not in bias:                   # PyTorch's non-capturable step: both corrections in Python doubles
                    bias[t] = (lr / (1 - beta1 ** t), (1 - beta2 ** t) ** 0.5)
                c[5].append(bias[t][0])
                c[6].append(bias[t][1])
                c[2].append(seen[5])
                c[3].append(seen[6])
                c[4].append(seen[7])
            c[0].extend(ps)
            c[1].extend(gs)
            c[7].append((decay, len(ps)))
        n_all = sum(len(c[0]) for c in calls.values())
        desc = np.empty(n_all, dtype=_DESC)
        spans, at, params, grads, decays = [], 0, [], [], []
        for key, c in calls.items():
            k = len(c[0])
            d = desc[at:at + k]
            d["p"] = [p.data_ptr() for p in c[0]]
            d["g"] = [g.data_ptr() for g in c[1]]
            d["m"], d["v"], d["n"], d["step_size"], d["bc2_sqrt"] = c[2], c[3], c[4], c[5], c[6]
            spans.append((key, at, k))
            params += c[0]
            grads += c[1]
            decays += c[7]                          # (factor, tensors) per group: the per-tensor list is made only where a factor is not 1
            at += k
        total = int(desc["n"].sum())
        base = desc.ctypes.data
        decay = np.repeat([x for x, _ in decays], [k for _, k in decays]).astype(np.float64) if any(x != 1.0 for x, _ in decays) else None
        # the average: the shadows of the parameters in the call travel with it, the other trainable parameters take the standalone launch
        ema, shadows, ema_w = self.ema, None, 0.0
        if ema is not None:
            ema_w = ema._advance()
            key = tuple(map(id, params))
            ent = self._ema_plans.get(key)
            ptrs = None if ent is None else [e.data_ptr() for e in ent[0]]
            if ent is None or ent[3] is not ema or ptrs != ent[2]:
                ent = self._plan_ema(key, ema, params, dev)
                ptrs = ent[2]
            fused_shadows, where, _, _, left = ent
            if fused_shadows:
                shadows = np.zeros(n_all, dtype=np.uint64)
                shadows[where] = ptrs
        clip = self.max_grad_norm is not None and self.max_grad_norm > 0
        skip = self.skip_nonfinite
        with torch.cuda.device(dev):
            stream = _native.stream_ptr()
            norm, ws, nbytes = None, None, 0
            if clip or skip:
                norm = torch.empty((), dtype=_F32, device=dev)
                nbytes = lib.dod_optim_workspace_bytes(n_all, total)
                if self._ws is None or self._ws.device != dev or self._ws.numel() < nbytes:
                    self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                ws = self._ws
                if skip and (self.skipped_steps is None or self.skipped_steps.device != dev):
                    self.skipped_steps = torch.zeros((), dtype=torch.int32, device=dev)
            one = len(spans) == 1
            if (clip or skip) and not one:
                # the norm runs over ALL groups once: the standalone clip (it writes the scaled gradients; max_norm = inf scales nothing),
                # then one unclipped update per call, each of which reads the stored norm when a non-finite one skips the step
                _check(lib.dod_optim_clip_grad_norm(base, n_all, self.max_grad_norm if clip else float("inf"), _native.ptr(norm), _native.ptr(ws),
                                                    nbytes, stream))
                params = params + grads
            o = self._options
            o.ema_w, o.skip_nonfinite, o.total_norm_dev = ema_w, int(skip), _native.ptr(norm)
            o.max_norm = self.max_grad_norm if clip and one else 0.0
            o.norm_ready = int(skip and not one)
            for j, ((beta1, beta2, eps, wd, _), first, count) in enumerate(spans):
                o.beta1, o.beta2, o.eps, o.weight_decay = beta1, beta2, eps, wd
                o.skipped_dev = _native.ptr(self.skipped_steps) if skip and j == 0 else None
                _check(lib.dod_optim_step(base + first * _DESC.itemsize, shadows.ctypes.data + 8 * first if shadows is not None else None,
                                          decay.ctypes.data + 8 * first if decay is not None else None, count, C.byref(o), _native.ptr(ws),
                                          nbytes, stream))
        if clip or skip:
            self.last_grad_norm = norm
        if ema is not None:
            params = params + fused_shadows
            left.run(ema_w)
        torch.autograd.graph.increment_version(params)

    def _plan_ema(self, key, ema, params, dev):
        """for the parameters of one step's call (key: their ids): (shadows that travel with the call, their positions, their data pointers,
        the average, the standalone launch of every other shadow) -- made once per set of parameters and again when a shadow's pointer moved"""
        shadow_of, in_call, fused, where, left = ema.shadow_of(), set(key), [], [], []
        for i, p in enumerate(params):
            e = shadow_of.get(id(p))
            if e is None:
                continue
            if _dense_f32_cuda(e) and e.device == dev and e.shape == p.shape:
                fused.append(e)
                where.append(i)
            else:
                left.append((e, p))
        left += [(e, p) for e, p in ema._pairs if id(p) not in in_call]
        if len(self._ema_plans) >= 8:                       # parameters whose gradient comes and goes: a few sets, not an unbounded number
            self._ema_plans.clear()
        ent = self._ema_plans[key] = (fused, np.asarray(where, dtype=np.intp), [e.data_ptr() for e in fused], ema, _Pairs(left))
        return ent


class AdamW(Adam, torch.optim.AdamW):
    """torch.optim.AdamW(...) plus `max_grad_norm`, `skip_nonfinite` and `ema`: `Adam` above with decoupled weight decay
    (`p *= 1 - lr * weight_decay` before the update, as a double factor per tensor), PyTorch's constructor defaults
    (`weight_decay=0.01`) and PyTorch's state, so `state_dict()` interchanges with `torch.optim.AdamW` both ways."""

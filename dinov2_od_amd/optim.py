"""The optimizer step of the training loop on the HIP kernels of csrc/optim.hip.

    from dinov2_od_amd.optim import Adam, clip_grad_norm_

`Adam` is `torch.optim.Adam` with one more argument, `max_grad_norm`: the reference's
`clip_grad_norm_(model.parameters(), gradient_clip_val)` + `optimizer.step()` (train.py:1101-1110) as
one call of two launches -- the gradients' sum of squares, then clip and update fused.  Its state
is PyTorch's (`step` CPU tensor, `exp_avg`, `exp_avg_sq`), so `state_dict()` / `load_state_dict()`
interchange with `torch.optim.Adam` in both directions.

The kernels take contiguous fp32 CUDA parameters with dense contiguous fp32 gradients on one
device, L2 weight decay, no amsgrad / maximize / capturable / differentiable / fused / tensor lr.
Every other configuration PyTorch accepts runs PyTorch's own step (after `clip_grad_norm_` below
when `max_grad_norm` is set): an explicit delegation of the cases the kernels do not implement,
never a substitute for a kernel that is missing -- on the native path a missing library raises.

The kernels write through `data_ptr()`, which autograd's version counters do not see; the engine
keys its packed weights on `(data_ptr, _version)` (engine.py), so every parameter (and every
gradient the standalone clip scales) is bumped with `torch.autograd.graph.increment_version`.
"""
import ctypes as C

import numpy as np
import torch

from . import _native

__all__ = ["Adam", "clip_grad_norm_"]

_F32, _STRIDED = torch.float32, torch.strided
# struct dod_optim_tensor as a numpy record: the step fills whole columns instead of 7 ctypes fields per tensor
_DESC = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i8"), ("step_size", "<f4"), ("bc2_sqrt", "<f4")])
assert _DESC.itemsize == C.sizeof(_native.DodOptimTensor)


def _check(rc):
    if rc != 0:
        msg = _native.lib().dod_optim_last_error()
        raise _native._EXC.get(rc, _native.DodError)(msg.decode() if msg else f"dinodet error {rc}")


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


class Adam(torch.optim.Adam):
    """torch.optim.Adam(...) plus `max_grad_norm` (None = no clipping).  `last_grad_norm`: the total gradient norm of the
    last step as a 0-dim device tensor (no synchronisation), None before the first clipped step."""

    def __init__(self, *args, max_grad_norm=None, **kwargs):
        super().__init__(*args, **kwargs)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.last_grad_norm = None
        # parameter -> (state dict, exp_avg, exp_avg_sq, step, numpy view of step, pointers of both moments, numel): the state is checked
        # once and again only when one of these objects has been replaced; the parameter and its fresh gradient are checked every step
        self._seen = {}
        self._ws = None

    def __getstate__(self):             # pickled / deep-copied: Optimizer keeps defaults, state and param_groups only
        state = super().__getstate__()
        state["max_grad_norm"] = self.max_grad_norm
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("max_grad_norm", None)
        self.__dict__.setdefault("last_grad_norm", None)
        self._seen, self._ws = {}, None

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
        """what the kernels need for this step, or None when PyTorch's step has to run: (device, [(key, params, grads, seen, lr)])
        with key = (beta1, beta2, eps, weight_decay), one entry per param group that has gradients"""
        if getattr(self, "grad_scale", None) is not None or getattr(self, "found_inf", None) is not None:
            return None
        plan, device, state, seen_of = [], None, self.state, self._seen
        for group in self.param_groups:
            if group["amsgrad"] or group["maximize"] or group["capturable"] or group["differentiable"] or group["fused"] \
                    or group.get("decoupled_weight_decay", False):
                return None
            lr, (beta1, beta2), eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
            if not all(isinstance(x, (int, float)) for x in (lr, beta1, beta2, eps, wd)):
                return None
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
                plan.append(((float(beta1), float(beta2), float(eps), float(wd)), ps, gs, ss, float(lr)))
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
            if self.max_grad_norm is not None and self.max_grad_norm > 0:
                self.last_grad_norm = clip_grad_norm_([p for g in self.param_groups for p in g["params"]], self.max_grad_norm)
            base = torch.optim.Adam.step
            if getattr(base, "hooked", False):      # this class's step already runs the step hooks
                base = base.__wrapped__
            base(self)
            return loss
        self._native_step(*plan)
        return loss

    def _native_step(self, dev, plan):
        lib = _native.lib()
        # one call per distinct (betas, eps, weight_decay); lr lives in the per-tensor step size, so groups that differ in lr alone share a call
        calls = {}
        for key, ps, gs, ss, lr in plan:
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
        n_all = sum(len(c[0]) for c in calls.values())
        desc = np.empty(n_all, dtype=_DESC)
        spans, at, params, grads = [], 0, [], []
        for key, c in calls.items():
            k = len(c[0])
            d = desc[at:at + k]
            d["p"] = [p.data_ptr() for p in c[0]]
            d["g"] = [g.data_ptr() for g in c[1]]
            d["m"], d["v"], d["n"], d["step_size"], d["bc2_sqrt"] = c[2], c[3], c[4], c[5], c[6]
            spans.append((key, at, k))
            params += c[0]
            grads += c[1]
            at += k
        total = int(desc["n"].sum())
        base = desc.ctypes.data
        clip = self.max_grad_norm is not None and self.max_grad_norm > 0
        with torch.cuda.device(dev):
            stream = _native.stream_ptr()
            norm, ws, nbytes = None, None, 0
            if clip:
                norm = torch.empty((), dtype=_F32, device=dev)
                nbytes = lib.dod_optim_workspace_bytes(n_all, total)
                if self._ws is None or self._ws.device != dev or self._ws.numel() < nbytes:
                    self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                ws = self._ws
            fused = self.max_grad_norm if clip and len(spans) == 1 else 0.0
            if clip and len(spans) > 1:
                # the norm runs over ALL groups once: the standalone clip (it writes the scaled gradients), then one unclipped update per call
                _check(lib.dod_optim_clip_grad_norm(base, n_all, self.max_grad_norm, _native.ptr(norm), _native.ptr(ws), nbytes, stream))
                params = params + grads
            for (beta1, beta2, eps, wd), first, count in spans:
                _check(lib.dod_optim_adam_step(base + first * _DESC.itemsize, count, beta1, beta2, eps, wd, fused, _native.ptr(norm), _native.ptr(ws),
                                               nbytes, stream))
        if clip:
            self.last_grad_norm = norm
        torch.autograd.graph.increment_version(params)

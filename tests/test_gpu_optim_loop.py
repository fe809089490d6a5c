"""dinov2_od_amd.optim.Adam in the training loop of tests/test_gpu_train_loop.py (cfg1, 112 x 112, 4 images, 8 steps): the loss
falls, the next eval() forward runs on the weights the kernels wrote (the engine keys its packed weights on the parameters'
version counters, which a write through data_ptr() leaves alone unless the step bumps them), and a state_dict() saved mid-run
resumes bit for bit."""
import copy

import numpy as np
import pytest
import torch

from dinov2_od_amd import _native as nat
from dinov2_od_amd import optim, synth
from tests import cases
from tests.test_gpu_train_loop import _loss

pytestmark = pytest.mark.gpu


def test_native_adam_in_the_training_loop():
    from dinov2_od_amd.matching import HungarianMatcher
    from tests import gpu_util as G
    torch.manual_seed(0)
    bb, dc = cases.cfg1(25)
    m = G.make_detector(bb, dc, "bf16", "facebook/dinov2-small")
    matcher = HungarianMatcher(per_image_rows=True)
    x = G.to_gpu(synth.make_pixels(4, 112, 112, seed=0))
    rng = np.random.default_rng(0)
    targets = []
    for b in range(4):
        n = int(rng.integers(1, 5))
        cxcy = 0.2 + 0.6 * rng.random((n, 2))
        wh = 0.1 + 0.2 * rng.random((n, 2))
        targets.append({"labels": torch.from_numpy(rng.integers(1, dc.num_classes, n)).cuda(),
                        "boxes": torch.from_numpy(np.concatenate([cxcy, wh], 1).astype(np.float32)).cuda()})
    m.eval()
    before = m.forward_packed(x).clone()          # the engine now holds weights packed from the initial parameters
    params = [p for p in m.parameters() if p.requires_grad]
    opt = optim.Adam(params, lr=2e-3, max_grad_norm=1.0)
    launches = nat.lib().dod_test_counter(b"optim_launches")
    losses, saved = [], None
    m.train()
    for step in range(8):
        out = m(x)
        idx = matcher({"pred_logits": out["pred_logits"].detach(), "pred_boxes": out["pred_boxes"].detach()}, targets)
        loss = _loss(out, targets, idx, dc.num_classes)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        if step == 4:                               # the state after step 4, the gradients of step 5
            saved = dict(state=copy.deepcopy(opt.state_dict()), params=[p.detach().clone() for p in params],
                         grads=[None if p.grad is None else p.grad.detach().clone() for p in params])
        opt.step()
        if step == 4:
            saved["after"] = [p.detach().clone() for p in params]
        losses.append(float(loss.detach()))
    with_grad = sum(g is not None for g in saved["grads"])
    per_step = sum(-(-with_grad // nat.lib().dod_test_counter(k)) for k in (b"optim_norm_table_tensors", b"optim_table_tensors"))
    assert nat.lib().dod_test_counter(b"optim_launches") - launches == 8 * per_step      # every step took the kernels
    assert all(np.isfinite(losses)) and bool(torch.isfinite(opt.last_grad_norm))
    assert min(losses[-3:]) < 0.8 * losses[0], losses

    m.eval()
    after = m.forward_packed(x).clone()
    assert torch.isfinite(after).all() and not torch.allclose(before, after)
    fresh = G.make_detector(bb, dc, "bf16", "facebook/dinov2-small")
    fresh.load_state_dict(m.state_dict())
    assert torch.equal(after, fresh.eval().forward_packed(x)), "the eval() forward ran on stale packed weights"

    resumed = [torch.nn.Parameter(p.clone()) for p in saved["params"]]
    opt2 = optim.Adam(resumed, lr=2e-3, max_grad_norm=1.0)
    opt2.load_state_dict(saved["state"])
    for p, g in zip(resumed, saved["grads"]):
        p.grad = g
    opt2.step()
    for p, want in zip(resumed, saved["after"]):
        assert torch.equal(p.detach(), want)

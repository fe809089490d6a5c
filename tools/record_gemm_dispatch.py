#!/usr/bin/env python3
"""Record what the inference GEMM launchers do at every case of tests/gemm_dispatch_cases.py: each case is launched once on zero-filled
buffers through the operator entry points, and the counters that moved (dod_test_counter: form_*, tail_splits, rem_cuts, f32_ksplits,
epi_regmath) are written with the device's CU count and the scratch reserved.  Stops at the first non-zero status.
tests/test_gemm_plan_cpu.py holds dod_test_gemm_plan to the file recorded at the commit before the planner arrived
(tests/golden/gemm_dispatch_parent.json).  Usage: python tools/record_gemm_dispatch.py OUT.json"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dinov2_od_amd import _native as nat
from tests import gemm_dispatch_cases as dc

SCRATCH = 64 << 20        # what dod_finalize_weights reserves
L = nat.lib()
dev = torch.device("cuda:0")
nat.check(L.dod_reserve_gemm_scratch(SCRATCH))
OUT_BYTES = {"f32": 4, "bf16": 2, "pair": 4, "h2": 4}
A_BYTES = {"bf16": 2, "x3": 4, "h2": 4, "fp8": 1, "f32": 4}           # operand bytes per element of K (activation rows)


def need(c):
    e = dc.EPI[c.epi]
    return c.M * c.K * A_BYTES[c.family], c.N * c.K * 4, c.M * c.N * OUT_BYTES[e.out]


sizes = [need(c) for c in dc.CASES]
A, W, O = [torch.zeros(max(s[i] for s in sizes) + 256, dtype=torch.uint8, device=dev) for i in range(3)]
vec = torch.zeros(max(c.N for c in dc.CASES), device=dev)                                  # bias, LayerScale, per-feature scales, weight exponents
rowsc = torch.zeros(max(c.M * max(c.K // 32, 4) for c in dc.CASES if c.family == "fp8"), dtype=torch.uint8, device=dev)      # per-row or block scales
outbs = torch.zeros(max(c.M * c.N // 64 for c in dc.CASES if c.family == "fp8"), dtype=torch.uint8, device=dev)
sp = nat.stream_ptr()
p = nat.ptr


def launch(c):
    e = dc.EPI[c.epi]
    M, N, K = c.M, c.N, c.K
    act = nat.ACT["swiglu_pairs" if e.glu and c.family != "fp8" else e.act]
    width = N // 2 if e.glu else N
    ldc = {"f32": width, "bf16": width, "pair": 2 * N, "h2": 2 * N}[e.out]
    resid, ldr = (p(O), ldc) if e.resid else (None, 0)                                     # in place, as the residual linears run
    scale = p(vec) if e.resid else None
    dt = nat.DOD_F32 if e.out == "f32" else nat.DOD_BF16
    layout = {"f32": 0, "bf16": 1, "pair": 2, "h2": 3}[e.out]
    if c.family in ("bf16", "f32"):
        return L.dod_op_linear(nat.DOD_BF16 if c.family == "bf16" else nat.DOD_F32, p(A), K, p(W), K, M, N, K, p(vec), scale, resid, ldr, p(O), dt, ldc, act, sp)
    if c.family == "x3":
        return L.dod_op_linear_x3(p(A), p(W), M, N, K, p(vec), scale, resid, ldr, p(O), layout, ldc, act, sp)
    if c.family == "h2":
        return L.dod_op_linear_h2(p(A), p(W), p(vec), M, N, K, p(vec), scale, resid, ldr, p(O), layout, ldc, act, sp)
    common = (M, N, K, p(vec), scale, resid, ldr, p(O), dt, ldc if not e.glu else N // 2, act)
    if e.scales == "rows":
        return L.dod_op_linear_fp8(p(A), K, p(rowsc), p(W), K, p(vec), *common, sp)
    if e.scales == "mx":
        return L.dod_op_linear_fp8_mx(p(A), K, p(rowsc), p(W), K, p(vec), *common, sp)
    return L.dod_op_linear_fp8_mx2(p(A), K, p(rowsc), p(W), K, p(W), *common, p(outbs) if e.glu else None, sp)


def snap():
    return {k: L.dod_test_counter(k.encode()) for k in dc.COUNTERS}


rec = []
for c in dc.CASES:
    nat.set_option("tailsplit", c.tailsplit)
    nat.set_option("f32_ksplit", c.f32_ksplit)
    before = snap()
    rc = launch(c)
    torch.cuda.synchronize()
    after = snap()
    if rc:
        print("stopped:", c, "status", rc, L.dod_last_error(None), flush=True)
        sys.exit(1)
    rec.append(dict(c._asdict(), moved={k: after[k] - before[k] for k in dc.COUNTERS if after[k] != before[k]}))
nat.set_option("tailsplit", -1)
nat.set_option("f32_ksplit", -1)
doc = {"cus": torch.cuda.get_device_properties(0).multi_processor_count, "scratch_bytes": SCRATCH, "cases": rec}
os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
with open(sys.argv[1], "w") as f:
    f.write("{\"cus\": %d, \"scratch_bytes\": %d, \"cases\": [\n" % (doc["cus"], SCRATCH) + ",\n".join(json.dumps(r) for r in rec) + "\n]}\n")
print(f"{len(rec)} cases recorded on {doc['cus']} CUs -> {sys.argv[1]}", flush=True)

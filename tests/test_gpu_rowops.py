"""`-m gpu`: the row and gather kernels between the GEMMs and attentions of every forward -- layernorm_kernel in each of its output forms,
rowstats_kernel, deform_sample_kernel with shared projections and the fused operand copy, swiglu_kernel and split3_kernel (rowops.hip,
deform.hip) -- through their operator entry points against float64, element by element.

tests/rowop_cases.py holds the inputs, the references, the bounds and the checks (tests/test_rowop_cases_cpu.py: what a CPU can show of
them, the seeded defects included); this file launches and collects:
  * every output sits between guard rows of a sentinel bit pattern and starts as another pattern that decodes to NaN (tests/gpu_util.Out,
    the scheme of tests/guard_rows.py with NaN inside): a store outside the rows, or a missing one, fails; every input sits between rows
    of NaN (gpu_util.guarded_input), so a read outside its rows turns an output to NaN;
  * every launch is made twice, into buffers of their own, and the two must agree bit for bit, guard rows included;
  * every violation of a case is collected before the test fails, and the worst share of each bound is printed per kernel and form when
    the module ends (DESIGN.md records them).
Shapes: rowop_cases.LN_D / LN_D_FREE name the dispatch arm of each D; all of them are a few rows."""
import functools

import pytest
import torch

from dinov2_od_amd import _native as nat
from tests import rowop_cases as rc
from tests.gpu_util import Out, guarded_input

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
WORST = {}          # (kernel, check) -> (share of the bound, where)
LN_OUTS = {"f32": ("f32", None), "bf16": ("bf16", None), "f32_bf16": ("f32", "bf16"), "pair": ("pair", None), "h2": ("h2", None),
           "fp8": ("q8", "scale"), "fp8_mx": ("q8", "bs"), "f32_s3": ("f32", "s3")}


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m 'not gpu' on CPU)")
    nat.lib()
    yield None
    for k in sorted(WORST):
        print(f"rowops worst  {k[0]:<22s} {k[1]:<22s} {WORST[k][0]:.3f} of its bound at {WORST[k][1]}")


def _dev(t, ld=None):
    return None if t is None else guarded_input(t.to(DEV), ld)


def _vec(t):
    return guarded_input(t.to(DEV)[None, :])


def _collect(kernel, where, res, outs, again, bad, count_unwritten=()):
    """the ratios of one launch into WORST, every violation into `bad`; outs / again: name -> Out of the two launches"""
    for name, val in res.items():
        if val >= WORST.get((kernel, name), (-1.0,))[0]:
            WORST[(kernel, name)] = (val, where)
        if not val <= 1.0:
            bad.append((kernel, where, name, val))
    for name, o in outs.items():
        if not o.guards_intact():
            bad.append((kernel, where, name, "guard rows or pad columns written"))
        if name in count_unwritten and o.unwritten():
            bad.append((kernel, where, name, f"{o.unwritten()} elements never written"))
        if not torch.equal(o.raw, again[name].raw):
            bad.append((kernel, where, name, "two launches differ"))


@functools.lru_cache(maxsize=None)
def _ln_case(D, vi):
    x, a, g, b, eps = rc.ln_input(D, rc.ln_variants(D)[vi])
    return (x, a, g, b, eps), rc.ln_reference(x, a, g, b, eps), (_dev(x), _dev(a), _vec(g), _vec(b))


def _ln_outs(form, rows, D):
    shape = {"f32": (D, F32), "bf16": (D, BF16), "pair": (2 * D, BF16), "h2": (4 * D, U8), "q8": (D, U8), "scale": (1, F32), "bs": (D // 32, U8),
             "s3": (3 * D, BF16)}
    return {n: Out(rows, shape[n][0], shape[n][1], unwritten=0xFF if n == "bs" else None) for n in LN_OUTS[form] if n}


def _ln_launch(form, dev, eps, rows, D):
    xd, ad, gd, bd = dev
    outs = _ln_outs(form, rows, D)
    o1, o2 = LN_OUTS[form]
    nat.check(nat.lib().dod_op_layernorm_form(nat.ptr(xd), nat.ptr(ad), nat.ptr(gd), nat.ptr(bd), eps, rows, D, nat.LN_FORM[form],
                                              nat.ptr(outs[o1].view), nat.ptr(outs[o2].view) if o2 else None, nat.stream_ptr()))
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("form", rc.LN_FORMS)
def test_layernorm_form(G, form):
    """one output form over every dispatch arm (D), 9 / 5 / 1 rows, both eps, with and without `add`, on normal, offset, outlier, constant
    and all-zero rows: every bound of rowop_cases.ln_check against the float64 reference"""
    bad = []
    for D in rc.ln_dims(form):
        for vi, variant in enumerate(rc.ln_variants(D)):
            (x, a, g, b, eps), R, dev = _ln_case(D, vi)
            rows = x.shape[0]
            outs, again = _ln_launch(form, dev, eps, rows, D), _ln_launch(form, dev, eps, rows, D)
            host = {n: (o.data.cpu()[:, 0] if n == "scale" else o.data.cpu()) for n, o in outs.items()}
            where = f"D={D} arm={rc.LN_ARMS[D]} {variant[0]} eps={eps} add={a is not None}"
            _collect(f"layernorm {form}", where, rc.ln_check(form, host, R), outs, again, bad, count_unwritten=set(outs) - {"h2"})
    assert not bad, bad


@pytest.mark.parametrize("kind", rc.RS_KINDS)
def test_rowstats(G, kind):
    """dod_op_rowstats over the same D sweep: (mean, rstd) against float64, the operand copy of x bit for bit"""
    family = {"bf16": nat.PREC["bf16"], "pair": nat.PREC["bf16x3"], "h2": nat.PREC["fp16x2"]}[kind]
    bad = []
    for D in rc.rs_dims(kind):
        width, dt = {"bf16": (D, BF16), "pair": (2 * D, BF16), "h2": (4 * D, U8)}[kind]
        for vi, variant in enumerate(rc.ln_variants(D)):
            (x, _, _, _, eps), _, dev = _ln_case(D, vi)
            rows = x.shape[0]
            R = rc.rs_reference(x, eps)
            runs = []
            for _ in range(2):
                outs = {"stats": Out(rows, 2, F32), "operand": Out(rows, width, dt)}
                nat.check(nat.lib().dod_op_rowstats(nat.ptr(dev[0]), rows, D, eps, nat.ptr(outs["operand"].view), family, nat.ptr(outs["stats"].view),
                                                    nat.stream_ptr()))
                torch.cuda.synchronize()
                runs.append(outs)
            res = rc.rs_check(kind, runs[0]["stats"].data.cpu(), runs[0]["operand"].data.cpu(), x, R)
            _collect(f"rowstats {kind}", f"D={D} arm={rc.RS_ARMS[D]} {variant[0]} eps={eps}", res, runs[0], runs[1], bad, count_unwritten={"stats"})
    assert not bad, bad


@pytest.mark.parametrize("case", rc.DF_CASES)
def test_deform_sample(G, case):
    """dod_op_deform_sample_ex: pitched projections with NaN pad columns, per-image and shared (Q rows, NaN behind them), with and without
    the fused [hi | hi | lo] copy, which must be the split of the same launch's fp32 rows bit for bit"""
    h, w, Hd, dh, P = case
    B, Q, N, Dd = rc.DF_B, rc.DF_Q, h * w, Hd * dh
    proj, values = rc.df_input(case)
    ldp = proj.shape[1]
    vd = _dev(values)
    bad = []
    for shared in (False, True):
        R = rc.df_reference(proj, values, case, shared)
        pd = _dev(proj[:Q] if shared else proj)              # the rows behind the Q shared ones are the input's NaN guard rows
        for with3 in (False, True):
            runs = []
            for _ in range(2):
                outs = {"out": Out(B * Q, Dd, F32)}
                if with3:
                    outs["out3"] = Out(B * Q, 3 * Dd, BF16)
                nat.check(nat.lib().dod_op_deform_sample_ex(nat.ptr(pd), ldp, int(shared), nat.ptr(vd), B, Q, N, Hd, P, dh, h, w, nat.ptr(outs["out"].view),
                                                            nat.ptr(outs["out3"].view) if with3 else None, nat.stream_ptr()))
                torch.cuda.synchronize()
                runs.append(outs)
            res = rc.df_check(runs[0]["out"].data.cpu(), runs[0]["out3"].data.cpu() if with3 else None, R)
            _collect(f"deform shared={int(shared)} out3={int(with3)}", f"{case}", res, runs[0], runs[1], bad, count_unwritten=set(runs[0]))
    assert not bad, bad


@pytest.mark.parametrize("rows,Fh", rc.SW_CASES)
@pytest.mark.parametrize("bf16", [False, True])
def test_swiglu(G, rows, Fh, bf16):
    """dod_op_swiglu, fp32 -> fp32 and bf16 -> bf16, gates at 0, +-20, +-88, +-89 (expf overflows between them), +-100 and +-1e4"""
    x = rc.sw_input(rows, Fh, bf16)
    R = rc.sw_reference(x, bf16)
    xd = _dev(x)
    runs = []
    for _ in range(2):
        outs = {"out": Out(rows, Fh, BF16 if bf16 else F32)}
        nat.check(nat.lib().dod_op_swiglu(nat.ptr(xd), nat.ptr(outs["out"].view), nat.DOD_BF16 if bf16 else nat.DOD_F32, rows, Fh, nat.stream_ptr()))
        torch.cuda.synchronize()
        runs.append(outs)
    bad = []
    res = {"out": rc.ratio(runs[0]["out"].data.cpu().double(), R["want"], R["bound"])}
    _collect(f"swiglu {'bf16' if bf16 else 'f32'}", f"{rows}x{Fh}", res, runs[0], runs[1], bad, count_unwritten={"out"})
    assert not bad, bad


@pytest.mark.parametrize("rows,K", rc.S3_CASES)
@pytest.mark.parametrize("weight_order", [0, 1])
def test_split3(G, rows, K, weight_order):
    """dod_op_split3 from a pitched input (NaN pad columns), both plane orders: the CPU split bit for bit"""
    x = rc.s3_input(rows, K)
    xd = _dev(x, K + rc.S3_PITCH_PAD)
    want = rc.s3_cpu(x, weight_order)
    runs = []
    for _ in range(2):
        outs = {"out": Out(rows, 3 * K, BF16)}
        nat.check(nat.lib().dod_op_split3(nat.ptr(xd), K + rc.S3_PITCH_PAD, rows, K, weight_order, nat.ptr(outs["out"].view), nat.stream_ptr()))
        torch.cuda.synchronize()
        runs.append(outs)
    bad = []
    got = runs[0]["out"].data.cpu()
    res = {"bits": 0.0 if torch.equal(got.view(torch.int16), want.view(torch.int16)) else rc.INF}
    _collect(f"split3 order={weight_order}", f"{rows}x{K}", res, runs[0], runs[1], bad, count_unwritten={"out"})
    assert not bad, bad

"""The banded matrix-core predictor (torchpiv_amd/csrc/predict_mfma.hip, every multipass Plan.run goes through it) where its
tile walk and its short bands run, against the HOST: float64 and long double products with the host's spline operators, a
derived error bound and the decision rule of the mask threshold (tests/predictor_model.py; its own checks, the numpy model of
the kernels and the mutants every case of the table has to catch: tests/test_predictor_model.py).

Per case of predictor_model.CASES: every batch, every mask of predictor_model.MASKS and both modes through Plan.debug_predict;
a batch below max_batch gives its pairs the bits they get inside the largest batch; a repeated call gives the same bits;
the dense kernel of engine.predict through the same checker; no write past the batch; and a plan whose passes have different
plane sizes gives pass 2 the same bits before and after pass 1 used the work buffer.

profiles/predictor_edges/README.md: what was observed on the device (error / bound per case, undecided cells, wall times)."""
import time

import numpy as np
import pytest
import torch

import predictor_model as PM

pytestmark = pytest.mark.gpu

IDS = [c["id"] for c in PM.CASES]
MODES = ("CWS", "DWS")
NAN_BITS = 0x7FF8DEAD0000BEEF          # a quiet NaN no kernel produces


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from torchpiv_amd import engine
    return engine


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()          # a copy: the model's cached inputs are read-only


def host(outs):
    return [o.cpu().numpy() for o in outs]


def make_plan(eng, c, mode):
    plan = eng.Plan(c["H"], c["W"], c["ws"], c["ov"], n_pass=c["n_pass"], mode=mode, pass_scale=c["pass_scale"],
                    max_batch=PM.max_batch(c), precision="fast")
    assert plan.geometry == [g[:4] for g in PM.passes(c)], (c["id"], plan.geometry)
    return plan


_UV = {}


def uv_reference(c, p, n):
    """Fields of u and v: they do not depend on the mask, so one pair of them serves every mask, mode and test."""
    key = (c["id"], p, n)
    if key not in _UV:
        Ay, Ax = PM.operators(c, p)
        u, v = PM.fields(c, p, n)
        _UV[key] = PM.Field(Ay, Ax, u), PM.Field(Ay, Ax, v)
    return _UV[key]


def reference(c, p, kind, n):
    Ay, Ax = PM.operators(c, p)
    return (*uv_reference(c, p, n), PM.Field(Ay, Ax, PM.mask(c, p, kind, n).astype(np.float64)))


def passed(tag, mode, ref, outs):
    st = PM.check(mode, ref, host(outs))
    assert st, tag + "\n  " + "\n  ".join(st.failures[:6])
    return st


class Seen:
    """What one test observed, printed as one line per mask (the numbers of the README)."""

    def __init__(self, what):
        self.what, self.ratio, self.und, self.t0 = what, 0.0, {}, time.perf_counter()

    def add(self, kind, st):
        self.ratio = max(self.ratio, st.ratio)
        u = self.und.setdefault(kind, [0, 0, 0])
        u[0], u[1], u[2] = u[0] + st.undecided, u[1] + st.undecided_masked, u[2] + st.cells

    def show(self):
        und = ", ".join(f"{k} {u[0]} ({u[1]} masked) of {u[2]}" for k, u in self.und.items() if u[0])
        print(f"  {self.what}: max |err| / bound {self.ratio:.3f}; undecided: {und or 'none'}; "
              f"{time.perf_counter() - self.t0:.2f} s")


@pytest.mark.parametrize("cid", IDS)
def test_banded_predictor_against_the_host_reference(eng, cid):
    c = PM.CASE[cid]
    n = PM.max_batch(c)
    seen = Seen(f"banded {cid}")
    for mode in MODES:
        plan = make_plan(eng, c, mode)
        for p in sorted(set(c["seq"])):
            u, v = (dev(t) for t in PM.fields(c, p, n))
            for kind in PM.MASKS:
                ref = reference(c, p, kind, n)
                m = dev(PM.mask(c, p, kind, n))
                big = None
                for b in sorted(c["batches"], reverse=True):
                    tag = f"{cid} pass {p} {mode} mask {kind} batch {b}"
                    outs = plan.debug_predict(p, u[:b], v[:b], m[:b])
                    if big is None:
                        big = outs
                    else:               # the same pairs inside the larger batch: other grids, another walk, the same bits
                        assert all(torch.equal(o, g[:b]) for o, g in zip(outs, big)), tag + ": differs from its pairs in batch " + str(n)
                    seen.add(kind, passed(tag, mode, ref, outs))
            again = plan.debug_predict(p, u, v, m)          # nothing in these kernels is atomic
            assert all(torch.equal(o, g) for o, g in zip(again, big)), f"{cid} pass {p} {mode}: a repeated call differs"
        plan.close()
    seen.show()


@pytest.mark.parametrize("cid", IDS)
def test_dense_predictor_against_the_host_reference(eng, cid):
    """engine.predict (the dense kernel, the yardstick of test_banded_predictor_equals_dense) on the first pairs of the same
    inputs, against the same reference by the same rule."""
    c = PM.CASE[cid]
    n = min(PM.max_batch(c), 8)
    seen = Seen(f"dense {cid}")
    for p in sorted(set(c["seq"])):
        Ay, Ax = (dev(t) for t in PM.operators(c, p))
        u, v = (dev(t) for t in PM.fields(c, p, n))
        for kind in PM.MASKS:
            ref = reference(c, p, kind, n)
            m = dev(PM.mask(c, p, kind, n))
            for mode in MODES:
                outs = eng.predict(mode, Ay, Ax, u, v, m)
                seen.add(kind, passed(f"dense {cid} pass {p} {mode} mask {kind}", mode, ref, outs))
    seen.show()


@pytest.mark.parametrize("mode", MODES)
def test_work_buffer_of_another_pass_leaves_no_trace(eng, mode):
    """stale_T1: pass 2 (T1 of 36 x 96 per field), pass 1 (17 x 64), pass 2 again on one plan."""
    c = PM.CASE["stale_T1"]
    n = PM.max_batch(c)
    plan = make_plan(eng, c, mode)
    for kind in ("r30", "half"):
        runs = []
        for p in c["seq"]:
            u, v = (dev(t) for t in PM.fields(c, p, n))
            outs = plan.debug_predict(p, u, v, dev(PM.mask(c, p, kind, n)))
            passed(f"stale_T1 pass {p} {mode} mask {kind}", mode, reference(c, p, kind, n), outs)
            runs.append(outs)
        assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[2])), f"{mode} {kind}: pass 2 differs after pass 1 ran"
    plan.close()


@pytest.mark.parametrize("cid", IDS)
def test_no_write_past_the_batch(eng, cid):
    """Output tensors one pair longer than the batch, prefilled with a NaN bit pattern: the extra pair keeps it, and the
    batch has the bits of the ordinary call."""
    from torchpiv_amd._lib import check, lib
    c = PM.CASE[cid]
    b = PM.max_batch(c)
    p = c["seq"][0]
    plan = make_plan(eng, c, "CWS")
    _, _, nr, nc = plan.geometry[p]
    u, v = (dev(t) for t in PM.fields(c, p, b))
    m = dev(PM.mask(c, p, "r30", b))
    want = plan.debug_predict(p, u, v, m)
    outs = [torch.full((b + 1, nr, nc), NAN_BITS, dtype=torch.int64, device="cuda").view(torch.float64) for _ in range(4)]
    assert all(torch.isnan(o).all() for o in outs)
    with torch.cuda.device(plan.device):
        check(lib.tpiv_plan_debug_predict(plan._h, p, b, u.data_ptr(), v.data_ptr(), m.data_ptr(),
                                          *[o.data_ptr() for o in outs], torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for name, o, w in zip(("u0", "v0", "u2", "v2"), outs, want):
        assert (o[b].view(torch.int64) == NAN_BITS).all(), f"{cid}: {name} written past pair {b - 1}"
        assert torch.equal(o[:b], w), f"{cid}: {name} differs from the ordinary call"
    plan.close()

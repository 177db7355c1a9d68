"""The stream contract of r2s_mesh_holes_dev (include/rho2sdf_hip.h, "Streams"), by the method of tests/test_stream_order_gpu.py,
whose helpers are copied here unchanged from tests/test_mesh_fans_stream_gpu.py (the first file's docstring explains them): the
expected result is computed the plain way (null stream, everything synchronised), then the same call is made in

  L  late producer: on a non-blocking stream S whose input buffers still hold a DECOY mesh of the same counts; a delay and then
     the copy of the real mesh are queued on S in front of the call; the outputs are poisoned;
  N  busy null stream: L with a longer delay queued on the null stream first,

and must give the plain call's bits, which differ from the decoy's.  The event behind the producer is asserted not done just
before the call.  The real input is ico_many_holes of tests/mesh_holes_cases.py (250 closed rims, all filled: 50 added vertices,
500 added triangles); the decoy has the same vertices and the same number of triangles, the first twelve of them collapsed (other
rims, other records, other totals, another fill).  Every group has room, so every output is written; the rows behind the counts
keep the poison."""
import ctypes
import time

import numpy as np
import pytest

import mesh_holes_cases as C

pytestmark = pytest.mark.gpu

vp = ctypes.c_void_p
MIN_DELAY_MS = 100.0   # (that file's 30 ms, raised: late in a long session the host once took longer than 30 ms to reach the call)
_cache = {}


def _p(t):
    return vp(t.data_ptr()) if t is not None else None


def _np_bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_np_bits(a), _np_bits(b))


def _poison(t):
    t.fill_(float("nan") if t.is_floating_point() else -7)
    return t


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


# ---- the delay ---------------------------------------------------------------------------------------------------------

def _delay(ms):
    """queue about `ms` milliseconds of work on the current stream: torch.cuda._sleep where it is usable, else a chain of
    matrix products on a scratch tensor; calibrated once with two events"""
    import torch
    if "delay" not in _cache:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        rate, kind = 0.0, "sleep"
        try:
            cycles = 20_000_000
            torch.cuda._sleep(1000)
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
            e1.synchronize()
            rate = cycles / max(e0.elapsed_time(e1), 1e-6)          # cycles per ms
            if cycles / rate < 1.0:                                 # returns at once: not usable on this device
                rate = 0.0
        except Exception:
            rate = 0.0
        if rate == 0.0:
            kind = "mm"
            a = torch.rand((2048, 2048), device="cuda:0")
            _cache["delay_scratch"] = (a, torch.empty_like(a))
            torch.mm(a, a, out=_cache["delay_scratch"][1])
            e0.record()
            for _ in range(16):
                torch.mm(a, a, out=_cache["delay_scratch"][1])
            e1.record()
            e1.synchronize()
            rate = 16 / max(e0.elapsed_time(e1), 1e-6)              # products per ms
        _cache["delay"] = (kind, rate)
        print(f"STREAM-ORDER delay: {kind}, {rate:.4g} units per ms")
    kind, rate = _cache["delay"]
    if kind == "sleep":
        torch.cuda._sleep(int(ms * rate))
    else:
        a, b = _cache["delay_scratch"]
        for _ in range(max(1, int(ms * rate))):
            torch.mm(a, a, out=b)


# ---- one entry point as a case ------------------------------------------------------------------------------------------

class Case:
    """name; real / decoy: lists of device tensors (same shapes); outputs(): fresh output tensors; call(ins, outs, stream) ->
    host scalars (a tuple compared with ==), `stream` a torch stream; result(ins, outs) -> the tensors that hold the result
    (in-place entry points: an input); prepare(): run before every call (the waiting regime of the plan)"""

    def __init__(self, name, real, decoy, outputs, call, result=None, prepare=None, keep=None):
        self.name, self.real, self.decoy, self.outputs, self.call = name, real, decoy, outputs, call
        self.result = result or (lambda ins, outs: outs)
        self.prepare = prepare or (lambda: None)
        self.keep = keep                                            # whatever must outlive the case (plans, indices, fields)
        self.expected = None


def _plain(case, ins):
    """the plain way: null stream, synchronised inputs, torch.cuda.synchronize() before reading -> (arrays, scalars, host ms)"""
    import torch
    bufs = [t.clone() for t in ins]
    outs = [_poison(o) for o in case.outputs()]
    case.prepare()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sc = case.call(bufs, outs, torch.cuda.default_stream())
    ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    return [r.cpu().numpy() for r in case.result(bufs, outs)], sc, ms


def _expected(case):
    """plain results of the real input and of the decoy, once per case; the first call is the warm one (workspaces grow
    there), the second is the one that is timed and kept"""
    if case.expected is None:
        _plain(case, case.real)
        real = _plain(case, case.real)
        decoy = _plain(case, case.decoy)
        again = _plain(case, case.real)                             # the warm state the scenarios start from
        assert again[1] == real[1] and all(_same(a, b) for a, b in zip(again[0], real[0])), f"{case.name}: the plain call does not repeat"
        differs = real[1] != decoy[1] or any(not _same(a, b) for a, b in zip(real[0], decoy[0]))
        assert differs or not case.real, f"{case.name}: the decoy's plain result equals the real one (a mistake in this test)"
        case.expected = dict(real=real[:2], decoy=decoy[:2], call_ms=max(real[2], again[2]))
    return case.expected


def _compare(label, got, sc, exp):
    (want, wsc), (dec, dsc) = exp["real"], exp["decoy"]
    ok = sc == wsc and all(_same(g, w) for g, w in zip(got, want))
    if ok:
        return
    on_decoy = sc == dsc and all(_same(g, d) for g, d in zip(got, dec))
    detail = []
    for k, (g, w) in enumerate(zip(got, want)):
        if not _same(g, w):
            gb, wb = _np_bits(g).ravel(), _np_bits(w).ravel()
            n = int((gb != wb).sum()) if gb.shape == wb.shape else -1
            pois = int(np.isnan(g).sum()) if g.dtype.kind == "f" else int((g == -7).sum())
            detail.append(f"output {k}: {n} of {gb.size} words differ, {pois} poisoned / NaN")
    if sc != wsc:
        detail.append(f"scalars {sc} != {wsc}")
    what = "ran on the decoy (the input copies queued on the stream were not waited for)" if on_decoy else \
        "stale, unwritten or mixed output"
    raise AssertionError(f"{label}: differs from the plain result - {what}; " + "; ".join(detail))


def _scenario(case, busy_null):
    """scenario L (busy_null False) or N (True), once; asserts the condition that makes it mean something, then bit equality"""
    import torch
    exp = _expected(case)
    delay_ms = max(5.0 * exp["call_ms"], MIN_DELAY_MS)
    bufs = [t.clone() for t in case.decoy]
    outs = [_poison(o) for o in case.outputs()]
    case.prepare()
    torch.cuda.synchronize()
    S = torch.cuda.Stream()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e_null = None
    if busy_null:
        _delay(2.0 * delay_ms + 5.0 * exp["call_ms"])              # outlasts the delay and the call on S
        e_null = torch.cuda.Event()
        e_null.record(torch.cuda.default_stream())
    with torch.cuda.stream(S):
        t0.record(S)
        _delay(delay_ms)
        t1.record(S)
        for b, r in zip(bufs, case.real):
            b.copy_(r, non_blocking=True)
        e_in = torch.cuda.Event()
        e_in.record(S)
        pending = not e_in.query() and (e_null is None or not e_null.query())
        sc = case.call(bufs, outs, S) if pending else None
        clones = [r.clone() for r in case.result(bufs, outs)] if pending else []
    S.synchronize()
    torch.cuda.synchronize()
    tag = "N" if busy_null else "L"
    assert pending, f"{case.name} {tag}: the producer had finished before the call was made - the scenario proves nothing"
    measured = t0.elapsed_time(t1)
    print(f"STREAM-ORDER {case.name} {tag}: plain call {exp['call_ms']:.2f} ms on the host, delay {measured:.1f} ms")
    _compare(f"{case.name} scenario {tag}", [c.cpu().numpy() for c in clones], sc, exp)


# ---- the holes -----------------------------------------------------------------------------------------------------------

def _holes_case(pkg):
    if "holes" in _cache:
        return _cache["holes"]
    import torch
    L, lib = pkg._lib, pkg._lib.lib()
    V, T = C.case("ico_many_holes")
    nv, nt = len(V), len(T)
    DT = T.copy()
    DT[:12] = 0                                                      # the decoy: the first twelve triangles collapsed
    rcap, ecap, vcap, tcap = 400, 1200, nv + 100, nt + 1000
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device="cuda:0")   # noqa: E731

    def holes(b, outs, st):
        sc = [ctypes.c_int64(-7) for _ in range(4)]
        r, tot = np.full(3, -7.0), np.full(8, -7, np.int64)
        L.check(lib.r2s_mesh_holes_dev(_p(b[0]), nv, _p(b[1]), nt, -1, _p(outs[0]), _p(outs[1]), _p(outs[2]), rcap, _p(outs[3]), ecap,
                                       _p(outs[4]), _p(outs[5]), vcap, tcap, *[ctypes.byref(x) for x in sc],
                                       r.ctypes.data_as(L.c_double_p), tot.ctypes.data_as(L.c_int64_p), vp(st.cuda_stream)))
        return tuple(x.value for x in sc) + (r.tobytes(), tot.tobytes())

    _cache["holes"] = Case("r2s_mesh_holes_dev", [_dev(V), _dev(T)], [_dev(V), _dev(DT)],
                           lambda: [e(rcap + 1, torch.int64), e((rcap, 8), torch.int64), e((rcap, 7), torch.float64), e(ecap, torch.int32),
                                    e((tcap, 3), torch.int32), e((vcap, 3), torch.float32)], holes)
    return _cache["holes"]


@pytest.mark.parametrize("busy_null", [False, True], ids=["L", "N"])
def test_mesh_holes_late_producer(pkg, busy_null):
    from test_mesh_holes_cpu import ref
    case = _holes_case(pkg)
    _scenario(case, busy_null)
    exp = case.expected
    assert exp["real"][1] != exp["decoy"][1], "the decoy's totals equal the real ones (a mistake in this test)"
    r = ref("ico_many_holes")                                        # (the real result is the restatement's)
    nt = len(C.case("ico_many_holes")[1])
    assert exp["real"][1][:4] == (250, 900, len(r["verts"]), len(r["tris"])) and exp["real"][1][5] == r["totals"].tobytes()
    assert (exp["real"][0][4][:nt + 500] == r["tris"]).all() and (exp["real"][0][3][:900] == r["rim_edge"]).all()
    assert (exp["real"][0][1][:250] == r["counts"]).all()

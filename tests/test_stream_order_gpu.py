"""The stream contract of the *_dev entry points (include/rho2sdf_hip.h, "Streams"): a call's work is ordered on the
caller's stream, its inputs need only be ready in stream order, and nothing is put on a stream the caller cannot order
against.  Every other GPU test passes the null stream with inputs and outputs fully synchronised, which cannot see a
launch or copy that went to the wrong stream, a missing event edge or per-call state reused too early.

Method: the expected result of every entry point is computed once the plain way (null stream, everything synchronised);
the same call is then made in the scenarios below and must give the same BITS (no tolerance: the same kernels on the same
data).

  L  late producer: the call is made on a non-blocking stream S whose input buffers still hold a DECOY (another valid input
     of the same shape whose plain result differs); a delay and then the copies of the real input are queued on S in front
     of the call.  A result equal to the decoy's plain result is reported as "ran on the decoy".
  N  busy null stream: L with a (longer) delay queued on the null stream first and the outputs poisoned (NaN / -7):
     internal work that went to the null stream finishes after the clones on S were taken.
  B  six calls back to back on one plan and one stream, alternating output sets, then alternating densities (the
     speculated sizes fail on every call and the device-side check falls back).
  P  two plans on two streams interleaved; one index / one field read from two streams at once.
  D  another device current (two devices and more): only the entry points whose behaviour in that situation the header
     documents - the others take pointers "on the current device", and calling them otherwise is outside the contract.

What makes L and N mean something is asserted, not measured: immediately before the entry point is called the event behind
the producer (and in N the one behind the null-stream delay) must not be done.  The delay is sized from the measured host
time of the plain call (five times, at least 30 ms).  Before every scenario one plain call with the same shapes has run on
the same plan / index / field / device, so no workspace grows inside the scenario (hipMalloc / hipFree wait for the whole
device and would hide an ordering fault); the library reports no allocation counters, the warm call is what guarantees it
(for the plan the list sizes of r2s_stats are compared as well).  Entry points that allocate scratch buffers on every call
(r2s_mesh_index_build_dev, r2s_rbf_smooth_dev without a workspace) can for that reason only show stale or unwritten
output, not an ordering fault.

The decoys are valid inputs (in-range indices, finite coordinates, the same counts, capacities sized for both): a stream
bug gives wrong numbers, never a wild address or a refusal."""
import ctypes
import time

import numpy as np
import pytest

from conftest import load_fixture

pytestmark = pytest.mark.gpu

vp = ctypes.c_void_p
MIN_DELAY_MS = 30.0
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


# ---- raw SDF: r2s_plan_run_dev and the tile exchange ---------------------------------------------------------------------

MODES = {"sdf": ("sdf",), "dist_sign_xp": ("dist", "sign", "xp")}


class PlanSetup:
    """one plan, one mesh on the device (HEX8: the sphere fixture at N_max = 10; TET4: the radial cube of
    test_parity_gpu.py::test_tet4_radial_cube), band factor 1.1, and the raw call through the C ABI (stats optional)"""

    def __init__(self, pkg, oracle, elem):
        from rho2sdf_jl_amd import synthetic
        self.pkg, self.L, self.elem = pkg, pkg._lib, elem
        if elem == "hex":
            X, IEN, rho = load_fixture("sphere")
            rn = oracle.dense_in_nodes(X, IEN, rho)
            self.grid = pkg.Grid(X.min(0), X.max(0), 10, 3)
            decoy = np.ascontiguousarray(rn[::-1])                  # the same mesh, nodal densities reversed
        else:
            X, IH, rn = synthetic.radial_cube(10, 10.0)
            IEN = synthetic.hex_to_tets(IH)
            self.grid = pkg.Grid(X.min(0), X.max(0), 40, 3)
            decoy = 1.0 - rn                                        # (the reversed field of this symmetric cube is the field itself)
        self.rho_t = 0.5
        self.real = [_dev(X), _dev(IEN), _dev(rn)]
        self.decoy = [_dev(X), _dev(IEN), _dev(decoy)]
        self.plan = pkg.DevicePlan(0)
        self.nx, self.ny, self.nz = self.grid.dims

    def planes(self, k_begin=0, k_end=None, zstride=1, zphase=0):
        from rho2sdf_jl_amd import slabs
        if zstride > 1:
            return 4 * slabs.interleaved_layers(self.nz, zstride, zphase)[0]
        return (self.nz if k_end is None else k_end) - k_begin

    def outputs(self, mode, **slab):
        import torch
        n = self.planes(**slab) * self.ny * self.nx
        return [torch.empty((n, 3) if k == "xp" else (n,), dtype=torch.float64, device="cuda:0") for k in MODES[mode]]

    def run(self, ins, outs, stream, mode, stats=None, k_begin=0, k_end=None, zstride=1, zphase=0):
        L = self.L
        p = L.R2SParams()
        L.lib().r2s_default_params(ctypes.byref(p))
        p.band_factor, p.elem_type, p.zstride, p.zphase = 1.1, (L.HEX8 if self.elem == "hex" else L.TET4), zstride, zphase
        o = dict(zip(MODES[mode], outs))
        bits = sum({"dist": L.OUT_DIST, "sign": L.OUT_SIGN, "sdf": L.OUT_SDF, "xp": L.OUT_XP}[k] for k in o)
        dX, dI, dR = ins
        L.check(L.lib().r2s_plan_run_dev(self.plan._h, _p(dX), dX.shape[0], _p(dI), dI.shape[0], _p(dR), self.rho_t,
                                         ctypes.byref(self.grid.c), ctypes.byref(p), k_begin, self.nz if k_end is None else k_end,
                                         bits, _p(o.get("dist")), _p(o.get("sign")), _p(o.get("sdf")), _p(o.get("xp")),
                                         vp(stream.cuda_stream), ctypes.byref(stats) if stats is not None else None))


def _plan_setup(pkg, oracle, elem, tag=""):
    key = ("plan", elem, tag)
    if key not in _cache:
        _cache[key] = PlanSetup(pkg, oracle, elem)
    return _cache[key]


def _plan_case(pkg, oracle, elem, mode, regime, slab=()):
    key = ("plan_case", elem, mode, regime, slab)
    if key in _cache:
        return _cache[key]
    import torch
    ps = _plan_setup(pkg, oracle, elem)
    slab_kw = dict(slab)

    def call(ins, outs, stream):
        ps.run(ins, outs, stream, mode, None, **slab_kw)            # stats = NULL: the call the benchmark and the slab path make
        return ()

    def prepare():
        # speculated regime: the previous call had the same shapes (every call of this case has).  Waiting regime:
        # R2S_NO_SPECULATION is read once per process, so a call with another k_end comes first - the next one reads its
        # sizes back in the middle
        st = ps.L.R2SStats()
        k_end = slab_kw.get("k_end", ps.nz)
        other = dict(slab_kw, k_end=k_end - 1) if regime == "waiting" else slab_kw
        ps.run(ps.real, ps.outputs(mode, **other), torch.cuda.default_stream(), mode, st, **other)
        torch.cuda.synchronize()
        if regime == "speculated":                                  # the same list sizes as ever: no workspace grows in the scenario
            sizes = (st.n_items, st.n_band_entries, st.n_sign_entries, st.n_tiles, st.n_active_tiles, st.n_iso_chunks)
            assert _cache.setdefault(key + ("sizes",), sizes) == sizes

    name = f"r2s_plan_run_dev {elem} {mode} {regime}" + (f" {slab_kw}" if slab_kw else "")
    _cache[key] = Case(name, ps.real, ps.decoy, lambda: ps.outputs(mode, **slab_kw), call, prepare=prepare, keep=ps)
    return _cache[key]


@pytest.mark.parametrize("busy_null", [False, True], ids=["L", "N"])
@pytest.mark.parametrize("regime", ["speculated", "waiting"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("elem", ["hex", "tet"])
def test_plan_run_late_producer(pkg, oracle, elem, mode, regime, busy_null):
    _scenario(_plan_case(pkg, oracle, elem, mode, regime), busy_null)


@pytest.mark.parametrize("busy_null", [False, True], ids=["L", "N"])
@pytest.mark.parametrize("slab", [(("k_begin", 4), ("k_end", 13)), (("zstride", 2), ("zphase", 1))], ids=["planes_4_13", "layers_1_of_2"])
def test_plan_run_slab_late_producer(pkg, oracle, slab, busy_null):
    """what the multi-GPU slab path runs: a contiguous slab that begins above plane 0, and interleaved tile layers"""
    case = _plan_case(pkg, oracle, "hex", "sdf", "speculated", slab)
    assert case.keep.nz >= 14
    _scenario(case, busy_null)


def _stitch_case(pkg, oracle):
    """r2s_fill_dev, r2s_plan_run_dev on the two interleaved halves, r2s_plan_pack_tiles_dev / r2s_unpack_tiles_dev,
    r2s_plan_pack_tiles2_dev / r2s_unpack_masks_dev and r2s_unpack_segments_dev: the sequence of
    test_parity_gpu.py::test_compressed_tile_stitching_equals_full_volume, queued on one stream end to end -> three stitched
    volumes (plain tiles, compressed tiles, the segment-wide scatter)"""
    if "stitch" in _cache:
        return _cache["stitch"]
    import torch
    from rho2sdf_jl_amd import slabs
    ps = _plan_setup(pkg, oracle, "hex", "stitch")
    L, lib, g, world = ps.L, ps.L.lib(), ps.grid, 2
    nvox = ps.nz * ps.ny * ps.nx
    # capacities that hold the real input and the decoy: a stream bug must not turn into a refusal
    cap = [0, 0, 0]
    for ins in (ps.real, ps.decoy):
        for r in range(world):
            st = L.R2SStats()
            ps.run(ins, ps.outputs("sdf", zstride=world, zphase=r), torch.cuda.default_stream(), "sdf", st, zstride=world, zphase=r)
            cap = [max(c, int(v)) for c, v in zip(cap, (st.n_active_tiles, st.n_sign_only_tiles, st.n_any_tiles))]
    mf, mm, ma = cap[0] + 3, cap[1] + 2, cap[2] + 1
    seglen = 2 + mf * 64 + (mf + 1) // 2 + mm + (mm + 1) // 2
    f64, i32, i64 = torch.float64, torch.int32, torch.int64

    def outputs():
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device="cuda:0")   # noqa: E731
        o = [e(nvox, f64) for _ in range(3)]                                  # the three stitched volumes
        for r in range(world):
            o += ps.outputs("sdf", zstride=world, zphase=r)
            o += [e(mf * 64, f64), e(mf, i32), e(mm, i64), e(mm, i32), e(ma * 64, f64), e(ma, i32)]
        return o + [e(world * seglen, f64)]

    def call(ins, outs, stream):
        s = vp(stream.cuda_stream)
        vol, vol_b, vol2, buf = outs[0], outs[1], outs[2], outs[-1]
        for v in (vol, vol_b, vol2):
            L.check(lib.r2s_fill_dev(_p(v), nvox, -1.0e10, s))
        L.check(lib.r2s_fill_dev(_p(buf), buf.numel(), 0.0, s))
        counts = []
        for r in range(world):
            local, payload, ids, masks, mids, payload_b, ids_b = outs[3 + 7 * r:10 + 7 * r]
            st = L.R2SStats()
            ps.run(ins, [local], stream, "sdf", st, zstride=world, zphase=r)
            nf, nm, na = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
            L.check(lib.r2s_plan_pack_tiles2_dev(ps.plan._h, _p(local), _p(payload), _p(ids), mf, _p(masks), _p(mids), mm,
                                                 ctypes.byref(nf), ctypes.byref(nm), s))
            L.check(lib.r2s_unpack_tiles_dev(_p(payload), _p(ids), nf.value, ctypes.byref(g.c), _p(vol), s))
            L.check(lib.r2s_unpack_masks_dev(_p(masks), _p(mids), nm.value, ctypes.byref(g.c), 1.0e10, _p(vol), s))
            L.check(lib.r2s_plan_pack_tiles_dev(ps.plan._h, _p(local), _p(payload_b), _p(ids_b), ma, ctypes.byref(na), s))
            L.check(lib.r2s_unpack_tiles_dev(_p(payload_b), _p(ids_b), na.value, ctypes.byref(g.c), _p(vol_b), s))
            assert (nf.value, nm.value, na.value) == (st.n_active_tiles, st.n_sign_only_tiles, st.n_any_tiles)
            counts += [nf.value, nm.value, na.value]
            # this rank's segment of the exchange buffer, laid out as slabs.SlabGather lays it out (torch copies on `stream`)
            with torch.cuda.stream(stream):
                seg = buf[r * seglen:(r + 1) * seglen]
                seg[:2].view(i64).copy_(torch.tensor([nf.value, nm.value]))
                p2, i2, m2, mi2 = slabs.SlabGather._segment_views(seg[2:], mf, mm)
                p2[:nf.value * 64].copy_(payload[:nf.value * 64]); i2[:nf.value].copy_(ids[:nf.value])
                m2[:nm.value].copy_(masks[:nm.value]); mi2[:nm.value].copy_(mids[:nm.value])
        L.check(lib.r2s_unpack_segments_dev(_p(buf), world, seglen, mf, mm, ctypes.byref(g.c), 1.0e10, _p(vol2), s))
        return tuple(counts)

    _cache["stitch"] = Case("tile exchange (fill, run, pack, pack2, unpack, masks, segments)", ps.real, ps.decoy, outputs, call,
                            result=lambda ins, outs: outs[:3], keep=ps)
    return _cache["stitch"]


@pytest.mark.parametrize("busy_null", [False, True], ids=["L", "N"])
def test_tile_exchange_late_producer(pkg, oracle, busy_null):
    import torch
    case = _stitch_case(pkg, oracle)
    exp = _expected(case)
    ps = case.keep
    full = ps.outputs("sdf")
    ps.run(ps.real, full, torch.cuda.default_stream(), "sdf")
    torch.cuda.synchronize()
    want = full[0].cpu().numpy()
    for k, v in enumerate(exp["real"][0]):
        assert _same(v, want), f"plain stitched volume {k} differs from the full-volume run"
    _scenario(case, busy_null)


def _run_six(ps, mode, S, inputs):
    """six calls on S with no host synchronisation of the test's own in between, alternating two poisoned output sets,
    a clone queued behind each -> the six results"""
    import torch
    sets = [[_poison(o) for o in ps.outputs(mode)] for _ in range(2)]
    torch.cuda.synchronize()
    clones = []
    with torch.cuda.stream(S):
        for i in range(6):
            ps.run(inputs[i % len(inputs)], sets[i % 2], S, mode)
            clones.append([o.clone() for o in sets[i % 2]])
            for o in sets[i % 2]:
                _poison(o)                                          # (queued behind the clone: the next user starts from poison)
    S.synchronize()
    return [[c.cpu().numpy() for c in cl] for cl in clones]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("elem", ["hex", "tet"])
def test_plan_run_back_to_back(pkg, oracle, elem, mode):
    """scenario B"""
    import torch
    case = _plan_case(pkg, oracle, elem, mode, "speculated")
    exp, ps = _expected(case), case.keep
    S = torch.cuda.Stream()
    case.prepare()
    for i, got in enumerate(_run_six(ps, mode, S, [ps.real])):
        _compare(f"{case.name} B, identical inputs, call {i}", got, (), exp)
    case.prepare()
    for i, got in enumerate(_run_six(ps, mode, S, [ps.real, ps.decoy])):   # the speculated sizes fail on every call from the second on
        which = "real" if i % 2 == 0 else "decoy"
        _compare(f"{case.name} B, alternating densities, call {i} ({which})", got, (),
                 dict(real=exp[which], decoy=exp["decoy" if which == "real" else "real"]))
    torch.cuda.synchronize()


def test_two_plans_on_two_streams(pkg, oracle):
    """scenario P: a HEX8 and a TET4 plan, one stream each, three calls each, queued alternately"""
    import torch
    cases = [_plan_case(pkg, oracle, elem, "sdf", "speculated") for elem in ("hex", "tet")]
    exps = [_expected(c) for c in cases]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for c in cases:
        c.prepare()
    outs = [[[_poison(o) for o in c.outputs()] for _ in range(3)] for c in cases]
    torch.cuda.synchronize()
    for i in range(3):
        for c, S, o in zip(cases, streams, outs):
            c.keep.run(c.real, o[i], S, "sdf")
    for S in streams:
        S.synchronize()
    for c, e, o in zip(cases, exps, outs):
        for i in range(3):
            _compare(f"{c.name} P, call {i}", [t.cpu().numpy() for t in o[i]], (), e)


def test_plan_run_with_another_device_current(pkg, oracle):
    """scenario D for r2s_plan_run_dev: the plan makes its own device current (r2s_plan_create's), whatever the caller had"""
    import torch
    if pkg._lib.lib().r2s_device_count() < 2 or torch.cuda.device_count() < 2:
        pytest.skip("one device only")
    case = _plan_case(pkg, oracle, "hex", "sdf", "speculated")
    exp, ps = _expected(case), case.keep
    case.prepare()
    outs = [_poison(o) for o in case.outputs()]
    S = torch.cuda.Stream(device=0)
    torch.cuda.synchronize()
    with torch.cuda.device(1):
        ps.run(ps.real, outs, S, "sdf")
    S.synchronize()
    _compare(f"{case.name} D", [o.cpu().numpy() for o in outs], (), exp)


# ---- post-processing ---------------------------------------------------------------------------------------------------------

def _noisy(pkg, seed):
    """the noisy field of test_stages_gpu.py::test_remove_artifacts_many_components cut from N_max = 70 to 36 (about
    39 x 27 x 20 points): several tiles in every direction and, counted with scipy.ndimage.label, 102 components for seed 23
    and 78 for seed 24; at N_max = 30 there are fewer than 64"""
    rng = np.random.default_rng(seed)
    pg = pkg.Grid(np.zeros(3), np.array([2.0, 1.3, 0.9]), 36, 1)
    nx, ny, nz = pg.dims
    f = rng.normal(size=(nz, ny, nx))
    for ax in range(3):
        f = f + np.roll(f, 1, axis=ax)
    return (f - 0.8).ravel(), pg


def _post_cases(pkg):
    if "post" in _cache:
        return _cache["post"]
    import torch
    L, lib = pkg._lib, pkg._lib.lib()
    (real, pg), (decoy, _) = _noisy(pkg, 23), _noisy(pkg, 24)
    ins, dec = [_dev(real)], [_dev(decoy)]
    CAP = 4096

    def remove(bufs, outs, stream):
        n = ctypes.c_int64(-7)
        L.check(lib.r2s_remove_artifacts_dev(_p(bufs[0]), ctypes.byref(pg.c), 0.0, 0.5, vp(stream.cuda_stream), ctypes.byref(n)))
        return (n.value,)

    def analyze(bufs, outs, stream):
        n = ctypes.c_int64(-7)
        roots, sizes = np.full(CAP, -7, np.int64), np.full(CAP, -7, np.int64)
        L.check(lib.r2s_analyze_components_dev(_p(bufs[0]), ctypes.byref(pg.c), 0.0, vp(stream.cuda_stream),
                                               roots.ctypes.data_as(L.c_int64_p), sizes.ctypes.data_as(L.c_int64_p), CAP, ctypes.byref(n)))
        assert 64 < n.value <= CAP, n.value
        return (n.value, roots.tobytes(), sizes.tobytes())

    inplace = lambda bufs, outs: [bufs[0]]   # noqa: E731
    _cache["post"] = {
        "remove_artifacts": Case("r2s_remove_artifacts_dev", ins, dec, lambda: [], remove, result=inplace),
        "analyze_components": Case("r2s_analyze_components_dev", ins, dec, lambda: [], analyze, result=inplace)}
    return _cache["post"]


def _rbf_case(pkg):
    """r2s_rbf_smooth_dev, interpolation on the refined grid: the (40, 23, 17) lattice of
    test_rbf_reference_gpu.py::test_rbf_refined_grid_tables_are_bit_identical"""
    if "rbf" in _cache:
        return _cache["rbf"]
    import torch
    from test_rbf_reference_gpu import _banded_spheres, _grid
    L, lib = pkg._lib, pkg._lib.lib()
    g = _grid(pkg, (40, 23, 17))
    (real, target), (decoy, _) = _banded_spheres(g, 11), _banded_spheres(g, 12)
    nf = int(np.prod([int(n) * 2 + 1 for n in g.c.N]))

    def call(bufs, outs, stream):
        th, its = ctypes.c_float(), ctypes.c_int32()
        L.check(lib.r2s_rbf_smooth_dev(_p(bufs[0]), ctypes.byref(g.c), 1, 2, 1e-3, float(target), _p(outs[0]), ctypes.byref(th),
                                       ctypes.byref(its), vp(stream.cuda_stream)))
        return (th.value, its.value)

    _cache["rbf"] = Case("r2s_rbf_smooth_dev", [_dev(real)], [_dev(decoy)],
                         lambda: [torch.empty(nf, dtype=torch.float32, device="cuda:0")], call)
    return _cache["rbf"]


@pytest.mark.parametrize("busy_null", [False, True], ids=["L", "N"])
@pytest.mark.parametrize("entry", ["remove_artifacts", "analyze_components", "rbf_smooth"])
def test_post_late_producer(pkg, entry, busy_null):
    _scenario(_rbf_case(pkg) if entry == "rbf_smooth" else _post_cases(pkg)[entry], busy_null)


# ---- the smoothed level-set as a function ----------------------------------------------------------------------------------

FIELD_ENTRIES = ["eval", "normals", "hessian", "curvature", "project"]


def _field_cases(pkg):
    """one fitted field on the smallest lattice of the field tests (test_field_hessian_gpu.py: 10 x 9 x 8 nodes), 4097 points:
    no multiple of the 16 lanes of a point group nor of the 256 threads of a block"""
    if "field" in _cache:
        return _cache["field"]
    import torch
    from test_field_gpu import _random_points
    from test_field_hessian_gpu import DIMS, _grid
    L, lib = pkg._lib, pkg._lib.lib()
    g = _grid(pkg)
    nx, ny, nz = DIMS
    ax = [g.AABB_min[a] + g.cell_size * np.arange(n) for a, n in enumerate(DIMS)]
    c = [0.5 * (a[0] + a[-1]) for a in ax]
    r = np.sqrt((ax[0][None, None, :] - c[0]) ** 2 + (ax[1][None, :, None] - c[1]) ** 2 + (ax[2][:, None, None] - c[2]) ** 2)
    sdf = (2.6 * g.cell_size - r).ravel()
    target = float((sdf > 0).mean()) * (nx - 1) * (ny - 1) * (nz - 1) * g.cell_size ** 3
    fld = pkg.fit_rbf_field(sdf, g, False, target, 1e-3, device=0)
    pts = [_random_points(g, np.random.default_rng(seed), 3600, 497) for seed in (5, 6)]
    assert all(len(p) == 4097 for p in pts)
    n = 4097
    real, decoy = [_dev(pts[0])], [_dev(pts[1])]
    h = fld._handle()
    e = lambda shape, dt=torch.float32: torch.empty(shape, dtype=dt, device="cuda:0")   # noqa: E731
    i32 = torch.int32
    tol = float(np.float32(1e-4 * g.cell_size))
    s = lambda stream: vp(stream.cuda_stream)   # noqa: E731
    calls = {
        "eval": (lambda: [e(n), e((n, 3)), e(n, i32)],
                 lambda b, o, st: L.check(lib.r2s_rbf_field_eval_dev(h, _p(b[0]), n, _p(o[0]), _p(o[1]), _p(o[2]), s(st))), None),
        "normals": (lambda: [e((n, 3))],
                    lambda b, o, st: L.check(lib.r2s_rbf_field_normals_dev(h, _p(b[0]), n, _p(o[0]), s(st))), None),
        "hessian": (lambda: [e(n), e((n, 3)), e((n, 6)), e(n, i32)],
                    lambda b, o, st: L.check(lib.r2s_rbf_field_hessian_dev(h, _p(b[0]), n, _p(o[0]), _p(o[1]), _p(o[2]), _p(o[3]), s(st))), None),
        "curvature": (lambda: [e((n, 4)), e((n, 3)), e((n, 6))],
                      lambda b, o, st: L.check(lib.r2s_rbf_field_curvature_dev(h, _p(b[0]), n, _p(o[0]), _p(o[1]), _p(o[2]), s(st))), None),
        "project": (lambda: [e(n, i32), e(n), e(n, i32)],
                    lambda b, o, st: L.check(lib.r2s_rbf_field_project_dev(h, _p(b[0]), n, 8, tol, _p(o[0]), _p(o[1]), _p(o[2]), s(st))),
                    lambda b, o: [b[0]] + o),                       # the points are moved in place
    }
    _cache["field"] = {}
    for k, (outs, fn, result) in calls.items():
        call = (lambda fn: lambda b, o, st: (fn(b, o, st), ())[1])(fn)
        _cache["field"][k] = Case(f"r2s_rbf_field_{k}_dev", real, decoy, outs, call, result=result, keep=fld)
    return _cache["field"]


@pytest.mark.parametrize("busy_null", [False, True], ids=["L", "N"])
@pytest.mark.parametrize("entry", FIELD_ENTRIES)
def test_field_late_producer(pkg, entry, busy_null):
    """the Python API passes torch's current stream: _scenario makes the call inside `with torch.cuda.stream(S)` and hands
    over that stream's handle, which is what api._stream(None) reads there"""
    _scenario(_field_cases(pkg)[entry], busy_null)


def _read_from_two_streams(label, call, points, outputs, want):
    """scenario P for an object that is only read: two streams, a delay at the head of each so that all six calls are
    queued before any of them runs, three calls each on its own point set, queued alternately"""
    import torch
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [[[_poison(o) for o in outputs()] for _ in range(3)] for _ in range(2)]
    torch.cuda.synchronize()
    events = []
    for S in streams:
        with torch.cuda.stream(S):
            _delay(MIN_DELAY_MS)
            events.append(torch.cuda.Event())
            events[-1].record(S)
    for i in range(3):
        for q, S in enumerate(streams):
            with torch.cuda.stream(S):
                call(points[q], outs[q][i], S)
    pending = not any(e.query() for e in events)
    for S in streams:
        S.synchronize()
    assert pending, f"{label}: a stream had run dry before the last call was queued - the scenario proves nothing"
    for q in range(2):
        for i in range(3):
            for k, (o, w) in enumerate(zip(outs[q][i], want[q])):
                assert _same(o.cpu().numpy(), w), f"{label}: stream {q}, call {i}, output {k} differs from the plain result"


def test_one_field_read_from_two_streams(pkg):
    cases = _field_cases(pkg)
    c = cases["eval"]
    exp = _expected(c)
    _read_from_two_streams("r2s_rbf_field_eval_dev", lambda p, o, S: c.call(p, o, S), [c.real, c.decoy], c.outputs,
                           [exp["real"][0], exp["decoy"][0]])


def test_field_with_another_device_current(pkg):
    """scenario D: the _dev entry points of a field refuse a call while another device is current (R2S_ERR_ARG, header),
    and leave the outputs alone"""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device only")
    for k, c in _field_cases(pkg).items():
        outs = [_poison(o) for o in c.outputs()]
        bufs = [t.clone() for t in c.real]
        torch.cuda.synchronize()
        with torch.cuda.device(1):
            with pytest.raises(pkg._lib.R2SError, match="device"):
                c.call(bufs, outs, torch.cuda.default_stream(0))
        torch.cuda.synchronize()
        for o in outs:
            a = o.cpu().numpy()
            assert (np.isnan(a) if a.dtype.kind == "f" else a == -7).all(), f"{c.name}: a refused call wrote to its outputs"
        assert torch.equal(bufs[0], c.real[0])


# ---- surface and mesh ---------------------------------------------------------------------------------------------------------

N24, DIMS24, ORIGIN24, H24 = 24, (24, 24, 24), (0.0, 0.0, 0.0), 1.0


def _lat24():
    return (ctypes.c_int64 * 3)(*DIMS24), (ctypes.c_double * 3)(*ORIGIN24)


def _sphere24(r, dtype):
    from test_isosurface_gpu import _sphere
    return _sphere(N24, r, dtype)


def _sphere_mesh(pkg, scale=1.0):
    """the extracted surface of the 24^3 sphere of radius 7; scale: the same triangles, vertices scaled about the centre"""
    from test_mesh_query_gpu import _surface
    if "mesh24" not in _cache:
        _cache["mesh24"] = _surface(pkg, _sphere24(7.0, np.float32), DIMS24, ORIGIN24, H24)
    V, T = _cache["mesh24"]
    c = np.float32((N24 - 1) / 2)
    return (c + (V - c) * np.float32(scale)).astype(np.float32), T


def _surface_cases(pkg):
    if "surface" in _cache:
        return _cache["surface"]
    import torch
    L, lib = pkg._lib, pkg._lib.lib()
    d, o = _lat24()
    nvox = N24 ** 3
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device="cuda:0")   # noqa: E731
    s = lambda stream: vp(stream.cuda_stream)   # noqa: E731
    cases = {}
    for name, dtype in (("float32", np.float32), ("float64", np.float64)):
        real, decoy = _sphere24(7.0, dtype), _sphere24(5.0, dtype)
        nv, nt = ctypes.c_int64(), ctypes.c_int64()
        L.check(lib.r2s_extract_isosurface(real.ctypes.data_as(vp), int(dtype == np.float32), d, o, H24, 0.0, 0, None, 0, None, 0,
                                           ctypes.byref(nv), ctypes.byref(nt)))
        vcap, tcap = nv.value + 2, nt.value + 2                     # (the smaller sphere needs less)

        def extract(b, outs, st, f32=int(dtype == np.float32), vcap=vcap, tcap=tcap):
            nv, nt = ctypes.c_int64(-7), ctypes.c_int64(-7)
            L.check(lib.r2s_extract_isosurface_dev(_p(b[0]), f32, d, o, H24, 0.0, _p(outs[0]), vcap, _p(outs[1]), tcap,
                                                   ctypes.byref(nv), ctypes.byref(nt), s(st)))
            return (nv.value, nt.value)

        cases[f"extract_{name}"] = Case(f"r2s_extract_isosurface_dev {name}", [_dev(real)], [_dev(decoy)],
                                        (lambda vcap=vcap, tcap=tcap: [e((vcap, 3), torch.float32), e((tcap, 3), torch.int32)]), extract)
    # the distance entry points: the decoy of a field is the sphere of the other radius, the decoy of a mesh the same
    # triangles on the smaller sphere (vertices scaled by 5 / 7 about the centre: equal counts)
    V, T = _sphere_mesh(pkg)
    V5, _ = _sphere_mesh(pkg, 5.0 / 7.0)
    band = 3.0

    def mesh_distance(b, outs, st):
        L.check(lib.r2s_mesh_distance_dev(_p(b[0]), len(V), _p(b[1]), len(T), d, o, H24, band, 0, _p(outs[0]), _p(outs[1]), s(st)))
        return ()

    cases["mesh_distance"] = Case("r2s_mesh_distance_dev", [_dev(V), _dev(T)], [_dev(V5), _dev(T)],
                                  lambda: [e(nvox, torch.float64), e(nvox, torch.int32)], mesh_distance)
    f64 = [_dev(_sphere24(7.0, np.float64))], [_dev(_sphere24(5.0, np.float64))]
    f32 = [_dev(_sphere24(7.0, np.float32))], [_dev(_sphere24(5.0, np.float32))]

    def redistance(b, outs, st):
        L.check(lib.r2s_redistance_dev(_p(b[0]), 0, d, o, H24, 0.0, band, _p(outs[0]), s(st)))
        return ()

    def redistance_full(b, outs, st):
        L.check(lib.r2s_redistance_full_dev(_p(b[0]), 1, d, o, H24, 0.0, _p(outs[0]), s(st)))
        return ()

    cases["redistance"] = Case("r2s_redistance_dev", f64[0], f64[1], lambda: [e(nvox, torch.float64)], redistance)
    cases["redistance_full"] = Case("r2s_redistance_full_dev", f32[0], f32[1], lambda: [e(nvox, torch.float32)], redistance_full)

    # the mesh index: built on the stream from the late mesh (decoy: vertices scaled by 0.5) and read back through the host
    # query; queried from 1025 late points; swept over the lattice
    Vh, _ = _sphere_mesh(pkg, 0.5)
    rng = np.random.default_rng(9)
    pts = [rng.uniform(-2.0, N24 + 1.0, (1025, 3)) for _ in range(2)]

    def build(b, outs, st):
        h = vp()
        L.check(lib.r2s_mesh_index_build_dev(_p(b[0]), len(V), _p(b[1]), len(T), s(st), ctypes.byref(h)))
        try:   # synchronous on return and owns a copy of the mesh: the host query reads what was built
            info = (ctypes.c_int64 * 4)()
            L.check(lib.r2s_mesh_index_info(h, info))
            dist, idx = np.full(1025, -7.0), np.full(1025, -7, np.int32)
            L.check(lib.r2s_mesh_index_query(h, pts[0].ctypes.data_as(vp), 0, 1025, 0, dist.ctypes.data_as(vp),
                                             idx.ctypes.data_as(L.c_int32_p)))
        finally:
            lib.r2s_mesh_index_destroy(h)
        return (tuple(info)[:3], dist.tobytes(), idx.tobytes())

    cases["index_build"] = Case("r2s_mesh_index_build_dev", [_dev(V), _dev(T)], [_dev(Vh), _dev(T)], lambda: [], build)
    ix = pkg.MeshIndex(V, T, device=0)
    h = ix._handle()

    def query(b, outs, st):
        L.check(lib.r2s_mesh_index_query_dev(h, _p(b[0]), 0, 1025, 0, _p(outs[0]), _p(outs[1]), s(st)))
        return ()

    def lattice(b, outs, st):
        L.check(lib.r2s_mesh_index_lattice_dev(h, d, o, H24, 0, _p(outs[0]), _p(outs[1]), s(st)))
        return ()

    cases["index_query"] = Case("r2s_mesh_index_query_dev", [_dev(pts[0])], [_dev(pts[1])],
                                lambda: [e(1025, torch.float64), e(1025, torch.int32)], query, keep=ix)
    cases["index_lattice"] = Case("r2s_mesh_index_lattice_dev", [], [], lambda: [e(nvox, torch.float64), e(nvox, torch.int32)],
                                  lattice, keep=ix)   # (no device input: the call must still queue behind the stream's delay)

    # mesh shells: no two recorded cases of tests/golden/mesh_shells_tris.npz have equal counts, so the decoy is the case with
    # its vertices mirrored in x (the same topology, other sums and another reference point)
    import mesh_shells_cases as MS
    Vs, Ts = (np.ascontiguousarray(a, dt) for a, dt in zip(MS.case("noise24_closed"), (np.float32, np.int32)))
    Vm = Vs.copy()
    Vm[:, 0] = -Vm[:, 0]
    ns = pkg.mesh_shells(Vs, Ts, device=0).n_shells
    assert ns > 1

    def shells(b, outs, st):
        n, ref, tot = ctypes.c_int64(-7), np.full(3, -7.0), np.full(8, -7, np.int64)
        L.check(lib.r2s_mesh_shells_dev(_p(b[0]), len(Vs), _p(b[1]), len(Ts), _p(outs[0]), _p(outs[1]), _p(outs[2]), ns,
                                        ctypes.byref(n), ref.ctypes.data_as(L.c_double_p), tot.ctypes.data_as(L.c_int64_p), s(st)))
        return (n.value, ref.tobytes(), tot.tobytes())

    cases["mesh_shells"] = Case("r2s_mesh_shells_dev", [_dev(Vs), _dev(Ts)], [_dev(Vm), _dev(Ts)],
                                lambda: [e(len(Ts), torch.int32), e((ns, 8), torch.int64), e((ns, 11), torch.float64)], shells)
    _cache["surface"] = cases
    return cases


SURFACE_ENTRIES = ["extract_float32", "extract_float64", "mesh_distance", "redistance", "redistance_full", "index_build",
                   "index_query", "index_lattice", "mesh_shells"]


@pytest.mark.parametrize("busy_null", [False, True], ids=["L", "N"])
@pytest.mark.parametrize("entry", SURFACE_ENTRIES)
def test_surface_and_mesh_late_producer(pkg, entry, busy_null):
    _scenario(_surface_cases(pkg)[entry], busy_null)


def test_one_index_read_from_two_streams(pkg):
    c = _surface_cases(pkg)["index_query"]
    exp = _expected(c)
    _read_from_two_streams("r2s_mesh_index_query_dev", lambda p, o, S: c.call(p, o, S), [c.real, c.decoy], c.outputs,
                           [exp["real"][0], exp["decoy"][0]])


def test_index_with_another_device_current(pkg):
    """scenario D: query_dev and lattice_dev refuse a call while another device than the index's is current (raycast_dev:
    test_ray_gpu.py)"""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device only")
    cases = _surface_cases(pkg)
    for k in ("index_query", "index_lattice"):
        c = cases[k]
        outs = [_poison(o) for o in c.outputs()]
        torch.cuda.synchronize()
        with torch.cuda.device(1):
            with pytest.raises(pkg._lib.R2SError, match="device"):
                c.call(c.real, outs, torch.cuda.default_stream(0))
        torch.cuda.synchronize()
        for o in outs:
            a = o.cpu().numpy()
            assert (np.isnan(a) if a.dtype.kind == "f" else a == -7).all(), f"{c.name}: a refused call wrote to its outputs"

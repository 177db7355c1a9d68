"""Cases and the child process of tests/test_threads_gpu.py: the threading contract of include/rho2sdf_hip.h ("sharing",
and "the calling thread's last ..." at every r2s_last_* function) with concurrent host threads.

Method, the same for every group (A shared field / index, B locked work-buffer families, C plans and host sessions,
D per-thread error state):

  serial      every call of the group once from the main thread on the default stream; one call per family is compared with
              its float64 / independent reference (iso_ref.vertices, mesh_dist_ref64, field_ref64, scipy.ndimage.label), so
              that "equal to serial" means "equal to the reference";
  concurrent  4 threads behind one barrier, each on a stream of its own, each running its own list of calls 8 times over and
              comparing every output with the serial one bit for bit.  The calls go through the package's wrappers, which
              read the thread's last table (r2s_last_components, _isosurface, _mesh_shells, ...) right after the call: a
              neighbour's table in its place is a differing output.  Every buffer the wrappers allocate for an output is
              filled with 0xFF bytes first (np.empty of the api module and torch.empty are wrapped in this process only);
  overlap     every call's entry and exit time (perf_counter) is kept; a round in which no two calls of different threads
              overlapped in time proves nothing and fails.  For the locked families an overlap of the host calls is the
              contended entry: the second caller had entered before the first one left;
  leak        r2s_live_device_bytes() after the group, with every handle destroyed and r2s_release_cache() run, equals its
              value before.

The library is loaded with ctypes.CDLL, which releases the interpreter lock for the length of every call, so the threads
do run inside the library at the same time.  Inputs differ between the threads in content and in size (thread 0 walks its
three sizes up, thread 1 down), so a per-device work buffer regrows between neighbouring calls.

Run as a script this file is the child: `thread_cases.py GROUP OUT.json`.
"""
import ctypes
import faulthandler
import json
import os
import sys
import threading
import time
import traceback

import numpy as np

N_THREADS = 4
REPEATS = 8
GROUPS = ("A", "B", "C", "D")
HANG_SECONDS = 150      # the child dumps every thread's stack and exits; the parent's own limit is 180 s
# thread -> the order in which it walks a family's three inputs (ascending size): 0 grows then shrinks, 1 the reverse
ORDERS = ((0, 1, 2, 1), (2, 1, 0, 1), (1, 2, 0), (2, 0, 1))


# ---------------------------------------------------------------------------------------------------------------------
# results as bits
# ---------------------------------------------------------------------------------------------------------------------
def flatten(obj, out=None):
    """every array of a (nested) result, in a fixed order, as contiguous numpy arrays; device tensors are copied back
    (which waits for the calling thread's current stream); timings (keys "ms_*") are left out"""
    out = [] if out is None else out
    if obj is None:
        out.append(np.zeros(0, np.uint8))
    elif isinstance(obj, np.ndarray):
        out.append(np.ascontiguousarray(obj))
    elif type(obj).__module__.startswith("torch"):
        out.append(np.ascontiguousarray(obj.cpu().numpy()))
    elif isinstance(obj, (bool, int, float, np.generic)):
        out.append(np.asarray([obj]))
    elif isinstance(obj, str):
        out.append(np.frombuffer(obj.encode(), np.uint8))
    elif isinstance(obj, dict):
        for k in obj:                       # (insertion order: the same code filled the dict in both passes)
            if not str(k).startswith("ms_"):
                flatten(k, out)
                flatten(obj[k], out)
    elif isinstance(obj, (tuple, list)):
        for v in obj:
            flatten(v, out)
    elif hasattr(obj, "__dict__"):          # MeshShells, MeshWeld, ...
        flatten(vars(obj), out)
    else:
        raise TypeError(f"cannot flatten {type(obj)}")
    return out


def _words(a):
    a = a.reshape(-1)
    if a.dtype.kind in "fc" or a.dtype.itemsize in (4, 8):
        return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64, 16: np.uint64}[a.dtype.itemsize])
    return a.view(np.uint8) if a.dtype.kind in "biu" else a


def differing(got, want):
    """number of differing words of two flattened results (NaN payloads and -0.0 count); a shape or type that differs
    counts every word"""
    if len(got) != len(want):
        return max(1, sum(w.size for w in want))
    n = 0
    for g, w in zip(got, want):
        if g.shape != w.shape or g.dtype != w.dtype:
            n += max(1, w.size)
        else:
            n += int((_words(g) != _words(w)).sum())
    return n


# ---------------------------------------------------------------------------------------------------------------------
# poisoned outputs
# ---------------------------------------------------------------------------------------------------------------------
class _PoisonedNumpy:
    """numpy, except that empty() comes back filled with 0xFF bytes (NaN / -1)"""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def empty(*args, **kw):
        a = np.empty(*args, **kw)
        a.reshape(-1).view(np.uint8)[...] = 0xFF
        return a


def poison_outputs(pkg):
    """every output the wrappers allocate starts as poison: the api module's np.empty, and torch.empty / empty_like"""
    import torch
    pkg.api.np = _PoisonedNumpy()
    empty, empty_like = torch.empty, torch.empty_like

    def fill(t):
        if t.is_cuda and t.numel():
            t.fill_(float("nan") if t.is_floating_point() else -1)
        return t

    torch.empty = lambda *a, **k: fill(empty(*a, **k))
    torch.empty_like = lambda *a, **k: fill(empty_like(*a, **k))


def poisoned(n, dtype=np.float64):
    a = np.empty(n, dtype)
    a.reshape(-1).view(np.uint8)[...] = 0xFF
    return a


def is_poison(a):
    return bool((np.ascontiguousarray(a).reshape(-1).view(np.uint8) == 0xFF).all())


# ---------------------------------------------------------------------------------------------------------------------
# calls, rounds and the two passes
# ---------------------------------------------------------------------------------------------------------------------
class Call:
    """key: names the call and its input (equal keys share one serial result); family: the label of the overlap report;
    fn() -> the result (anything flatten takes)"""

    def __init__(self, key, family, fn):
        self.key, self.family, self.fn = key, family, fn


class Round:
    """lists[t]: the calls of thread t (an empty list: the thread sits the round out)"""

    def __init__(self, name, lists, repeats=REPEATS):
        self.name, self.lists, self.repeats = name, lists, repeats


def serial_pass(rounds, expected):
    import torch
    t0 = time.perf_counter()
    for r in rounds:
        for calls in r.lists:
            for c in calls:
                if c.key not in expected:
                    expected[c.key] = flatten(c.fn())
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _worker(tid, calls, repeats, expected, barrier, rec):
    import torch
    try:
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            barrier.wait()
            for _ in range(repeats):
                for c in calls:
                    t0 = time.perf_counter()
                    res = c.fn()
                    t1 = time.perf_counter()
                    rec["spans"].append((t0, t1))
                    n = differing(flatten(res), expected[c.key])
                    rec["compared"] += 1
                    if n:
                        rec["differ_calls"] += 1
                        rec["differ_words"] += n
                        if len(rec["notes"]) < 5:
                            rec["notes"].append(f"thread {tid} {c.key}: {n} words differ from the serial result")
            stream.synchronize()
    except BaseException:   # noqa: BLE001  (reported by the main thread)
        rec["error"] = traceback.format_exc()
        barrier.abort()


def overlaps(spans):
    """number of pairs of calls of different threads whose [entry, exit] intervals intersect"""
    ev = sorted((s[0], s[1], t) for t, sp in enumerate(spans) for s in sp)
    n = 0
    for i, (a0, a1, ta) in enumerate(ev):
        for b0, _, tb in ev[i + 1:]:
            if b0 >= a1:
                break
            n += ta != tb
    return n


def concurrent_pass(rounds, expected):
    """-> (seconds, report per round); raises on a worker's exception"""
    report = []
    t_all = time.perf_counter()
    for r in rounds:
        active = [t for t in range(N_THREADS) if r.lists[t]]
        barrier = threading.Barrier(len(active))
        recs = {t: dict(spans=[], compared=0, differ_calls=0, differ_words=0, notes=[], error=None) for t in active}
        threads = [threading.Thread(target=_worker, args=(t, r.lists[t], r.repeats, expected, barrier, recs[t])) for t in active]
        t0 = time.perf_counter()
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        errors = [recs[t]["error"] for t in active if recs[t]["error"] and "BrokenBarrierError" not in recs[t]["error"]]
        if errors:
            raise RuntimeError(f"round {r.name}: a worker raised\n" + "\n".join(errors))
        report.append(dict(round=r.name, threads=len(active), seconds=round(time.perf_counter() - t0, 3),
                           compared=sum(recs[t]["compared"] for t in active),
                           differ_calls=sum(recs[t]["differ_calls"] for t in active),
                           differ_words=sum(recs[t]["differ_words"] for t in active),
                           overlaps=overlaps([recs[t]["spans"] for t in active]),
                           notes=[n for t in active for n in recs[t]["notes"]]))
    return time.perf_counter() - t_all, report


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
LO, H = np.array([0.013, -0.2, 0.07]), 0.1037   # the non-dyadic lattice of test_field_gpu.py


def lattice_grid(pkg, dims, h=H):
    """a Grid whose lattice has exactly `dims` points (test_field_gpu._grid)"""
    dims = np.array(dims)
    g = pkg.Grid(LO, LO + h * (dims - 1.0), int(dims.max()) - 1, 0)
    assert g.dims == tuple(int(d) for d in dims)
    return g


def lattice_of(g):
    return g.dims, tuple(g.c.aabb_min[:]), float(g.cell_size)


def fields(pkg):
    """three float32 fields of ascending size and different content -> [(grid, values (nz, ny, nx))]: a gyroid (open at the
    lattice border), noise with an exterior border (many small bodies), a ball"""
    import iso_ref
    import mesh_query_cases as Q
    import mesh_shells_cases as S
    return [(lattice_grid(pkg, (17, 17, 17)), iso_ref.gyroid(17, 12)),
            (lattice_grid(pkg, (24, 24, 24)), S.noise_field().reshape(24, 24, 24)),
            (lattice_grid(pkg, (33, 33, 33)), Q.sphere_field(33, 9.0, np.float32).reshape(33, 33, 33))]


def ball_sdf(g, radius_cells, centre=(0.5, 0.5, 0.5)):
    """float64 signed distance (positive inside) to a ball on the lattice of `g`, flattened x fastest"""
    nx, ny, nz = g.dims
    amin, h = np.array(g.c.aabb_min[:]), float(g.cell_size)
    z, y, x = np.meshgrid(*(amin[a] + h * np.arange(n) for a, n in ((2, nz), (1, ny), (0, nx))), indexing="ij")
    c = amin + h * (np.array([nx, ny, nz]) - 1.0) * np.array(centre)
    return (radius_cells * h - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)).ravel()


def points_in(g, n, seed, margin=2.0):
    """n float32 points in the box of `g` widened by `margin` cells, and a NaN row"""
    amin, amax, h = np.array(g.c.aabb_min[:]), np.array(g.c.aabb_max[:]), float(g.cell_size)
    p = (amin - margin * h + np.random.default_rng(seed).random((n, 3)) * (amax - amin + 2 * margin * h)).astype(np.float32)
    p[n // 2] = np.nan
    return p


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------
# group A: one shared field / index, many readers
# ---------------------------------------------------------------------------------------------------------------------
def field_calls(tag, f, pts):
    d = dev(pts)
    tol = np.float32(1e-3)
    return [Call(f"{tag} eval", "field", lambda: f.eval(pts, grad=True, taps=True)),
            Call(f"{tag} eval_dev", "field", lambda: f.eval_dev(d, grad=True, taps=True)),
            Call(f"{tag} hessian", "field", lambda: f.eval(pts, hess=True, taps=True)),
            Call(f"{tag} hessian_dev", "field", lambda: f.hessian_dev(d, taps=True)),
            Call(f"{tag} normals", "field", lambda: f.normals(pts)),
            Call(f"{tag} normals_dev", "field", lambda: f.normals_dev(d)),
            Call(f"{tag} curvature", "field", lambda: np.stack(f.curvature(pts), axis=1)),
            Call(f"{tag} curvature_dev", "field", lambda: f.curvature_dev(d)),
            Call(f"{tag} project", "field", lambda: f.project(pts, 6, tol)),
            Call(f"{tag} project_dev", "field", lambda: f.project_dev(d, 6, tol))]


def index_calls(tag, ix, pts, lat):
    rng = np.random.default_rng(len(pts))
    dirs = rng.normal(size=pts.shape).astype(np.float32)
    d, dd = dev(pts), dev(dirs)
    return [Call(f"{tag} query", "index", lambda: ix.distance(pts, want_index=True)),
            Call(f"{tag} query_dev", "index", lambda: ix.distance_dev(d, want_index=True)),
            Call(f"{tag} lattice", "index", lambda: ix.lattice(lat, want_index=True)),
            Call(f"{tag} lattice_dev", "index", lambda: ix.lattice_dev(lat, want_index=True)),
            Call(f"{tag} raycast", "index", lambda: ix.raycast(pts, dirs, want_index=True, want_side=True)),
            Call(f"{tag} raycast_dev", "index", lambda: ix.raycast_dev(d, dd, want_index=True, want_side=True)),
            Call(f"{tag} winding", "index", lambda: ix.winding(pts, want_crossings=True)),
            Call(f"{tag} winding_dev", "index", lambda: ix.winding_dev(d, want_crossings=True)),
            Call(f"{tag} winding_lattice", "index", lambda: ix.winding_lattice(lat, want_crossings=True)),
            Call(f"{tag} winding_lattice_dev", "index", lambda: ix.winding_lattice_dev(lat, want_crossings=True)),
            Call(f"{tag} signed", "index", lambda: ix.signed_distance(pts, want_index=True)),
            Call(f"{tag} signed_dev", "index", lambda: ix.signed_distance_dev(d, want_index=True)),
            Call(f"{tag} signed_lattice", "index", lambda: ix.signed_lattice(lat, want_index=True)),
            Call(f"{tag} signed_lattice_dev", "index", lambda: ix.signed_lattice_dev(lat, want_index=True))]


class SharedObjects:
    """field 1: fitted on the 20 x 17 x 22 lattice; field 2: random weights on 12 x 15 x 11; index 1: the extracted ball
    (about 2000 triangles); index 2: the extracted gyroid"""

    def __init__(self, pkg):
        self.pkg = pkg
        self.g1, self.g2 = lattice_grid(pkg, (20, 17, 22)), lattice_grid(pkg, (12, 15, 11))
        sdf = ball_sdf(self.g1, 6.3)
        target = 4.0 / 3.0 * np.pi * (6.3 * H) ** 3
        self.f1 = pkg.fit_rbf_field(sdf, self.g1, True, target, 1e-3, device=0)
        nx, ny, nz = self.g2.dims
        self.w2 = np.random.default_rng(7).standard_normal((nz, ny, nx)).astype(np.float32)
        self.f2 = pkg.RbfField(self.w2, self.g2, -0.11, 1e-3, device=0)
        fl = fields(pkg)
        self.mesh1 = pkg.extract_isosurface(fl[2][1], fl[2][0], device=0)
        self.mesh2 = pkg.extract_isosurface(fl[0][1], fl[0][0], device=0)
        self.box1, self.box2 = fl[2][0], fl[0][0]
        self.ix1, self.ix2 = pkg.MeshIndex(*self.mesh1, device=0), pkg.MeshIndex(*self.mesh2, device=0)

    def lists(self):
        """thread t: its own points (disjoint sets of different sizes) and lattice; threads 2 and 3 alternate between the
        two fields and the two indices call by call"""
        sizes = (3001, 1700, 901, 2500)
        lists = []
        for t in range(N_THREADS):
            lat = ((9 + t, 11, 10 + t), tuple(LO - 0.2 * t), 0.4 + 0.05 * t)
            a = field_calls(f"t{t} field1", self.f1, points_in(self.g1, sizes[t], 100 + t)) \
                + index_calls(f"t{t} index1", self.ix1, points_in(self.box1, sizes[t], 200 + t), lat)
            if t >= 2:
                b = field_calls(f"t{t} field2", self.f2, points_in(self.g2, sizes[t] // 2, 300 + t)) \
                    + index_calls(f"t{t} index2", self.ix2, points_in(self.box2, sizes[t] // 2, 400 + t), lat)
                a = [c for pair in zip(a, b) for c in pair]
            lists.append(a)
        return lists

    def check_reference(self, expected):
        """one call per family of the serial pass against its float64 reference"""
        import field_ref64 as F
        import mesh_dist_ref64 as M
        g, pts = self.g2, points_in(self.g2, 2500 // 2, 303)
        val = expected["t3 field2 eval"][0]
        fld = F.Field(self.w2, np.array(g.c.aabb_min[:]), np.array(g.c.aabb_max[:]), [int(n) for n in g.c.N], float(g.c.cell_size),
                      1e-3, np.float32(-0.11))
        ref = fld.evaluate(pts)
        fin = np.isfinite(ref["val"])
        err, vb = np.abs(val.astype(np.float64) - ref["val"]), fld.value_bound(ref)
        assert fin.sum() >= len(pts) - 1 and np.isnan(val[~fin]).all() and (err[fin] <= vb[fin]).all(), "field eval vs field_ref64"
        V, T = self.mesh1
        P = points_in(self.box1, 901, 202).astype(np.float64)
        d, idx = expected["t2 index1 query"][:2]
        fin = np.isfinite(P).all(axis=1)
        dr, _ = M.distance_brute(V, T, P[fin])
        L = max(float(np.abs(P[fin]).max()), float(np.abs(V).max()))
        assert (np.abs(d[fin] - dr) <= M.bound(dr, L, np.float64)).all() and np.isnan(d[~fin]).all(), "index query vs mesh_dist_ref64"
        assert ((idx[fin] >= 0) & (idx[fin] < len(T))).all()
        assert 1000 <= len(T) <= 4000, len(T)   # ("about 2000 triangles")

    def close(self):
        for o in (self.f1, self.f2, self.ix1, self.ix2):
            o.close()


def group_a(pkg):
    so = SharedObjects(pkg)
    return [Round("shared field and index", so.lists())], so.check_reference, so.close


# ---------------------------------------------------------------------------------------------------------------------
# group B: the families that lock a per-device work cache
# ---------------------------------------------------------------------------------------------------------------------
def components_dev(pkg, d_sdf, grid):
    """r2s_analyze_components_dev: count, then the table; and the thread's last table -> four arrays"""
    L, lib = pkg._lib, pkg._lib.lib()
    n = ctypes.c_int64(-1)
    st = pkg.api._stream(None)
    ip = lambda a: a.ctypes.data_as(L.c_int64_p)   # noqa: E731
    L.check(lib.r2s_analyze_components_dev(ctypes.c_void_p(d_sdf.data_ptr()), ctypes.byref(grid.c), 0.0, st, None, None, 0, ctypes.byref(n)))
    roots, sizes = poisoned(n.value, np.int64), poisoned(n.value, np.int64)
    L.check(lib.r2s_analyze_components_dev(ctypes.c_void_p(d_sdf.data_ptr()), ctypes.byref(grid.c), 0.0, st, ip(roots), ip(sizes), n.value,
                                           ctypes.byref(n)))
    lr, ls = poisoned(n.value, np.int64), poisoned(n.value, np.int64)
    L.check(lib.r2s_last_components(ip(lr), ip(ls), n.value, ctypes.byref(n)))
    return roots, sizes, lr, ls


def remove_dev(pkg, d_sdf, grid):
    """r2s_remove_artifacts_dev on a copy -> (n flipped, the field)"""
    L, lib = pkg._lib, pkg._lib.lib()
    d = d_sdf.clone()
    n = ctypes.c_int64(-1)
    L.check(lib.r2s_remove_artifacts_dev(ctypes.c_void_p(d.data_ptr()), ctypes.byref(grid.c), 0.0, 0.01, pkg.api._stream(None), ctypes.byref(n)))
    return int(n.value), d


def remove_host(pkg, sdf, grid):
    a = sdf.copy()
    return pkg.remove_sdf_artifacts(a, grid, device=0), a


def smoothing(pkg, sdf, grid, smooth, target):
    info = {}
    fine = pkg.RBFs_smoothing(sdf, grid, True, smooth, target, 1e-3, device=0, info=info)
    return fine, info, pkg.last_rbf_plan()


class Families:
    """name -> three calls lists (one per input, ascending size), host and _dev form of each entry point"""

    def __init__(self, pkg):
        self.pkg = pkg
        self.fields = fields(pkg)
        self.meshes = [pkg.extract_isosurface(v, g, device=0) for g, v in self.fields]
        self.by_input = {}
        self.smooth_inputs = []
        fam = self.by_input
        for k, ((g, v), (V, T)) in enumerate(zip(self.fields, self.meshes)):
            f64, d32, d64 = v.astype(np.float64).ravel(), dev(v), dev(v.astype(np.float64))
            dV, dT = dev(V), dev(T)
            band = 3.0 * float(g.cell_size)
            lat = lattice_of(g)
            soup = np.ascontiguousarray(V[T.ravel()])
            d_soup = dev(soup)
            snap = float(g.cell_size) / 8
            levels = float(g.c.aabb_min[2]) + float(g.cell_size) * np.array([2.5, 7.25, 11.0, 15.5])
            C = lambda name, family, fn: fam.setdefault(family, [[], [], []])[k].append(Call(f"{name} #{k}", family, fn))   # noqa: E731
            C("remove_artifacts", "components", lambda f64=f64, g=g: remove_host(pkg, f64, g))
            C("remove_artifacts_dev", "components", lambda d64=d64, g=g: remove_dev(pkg, d64, g))
            C("analyze_components", "components", lambda f64=f64, g=g: pkg.analyze_sdf_components(f64, g, device=0))
            C("analyze_components_dev", "components", lambda d64=d64, g=g: components_dev(pkg, d64, g))
            C("extract_isosurface", "extract", lambda v=v, g=g: pkg.extract_isosurface(v, g, device=0))
            C("extract_isosurface_dev", "extract", lambda d32=d32, g=g: pkg.extract_isosurface_dev(d32, g))
            C("redistance", "redistance", lambda v=v, g=g, band=band: pkg.redistance(v, g, band=band, device=0))
            C("redistance_dev", "redistance", lambda d32=d32, g=g, band=band: pkg.redistance_dev(d32, g, band=band))
            C("redistance_full", "redistance_full", lambda v=v, g=g: pkg.redistance_full(v, g, device=0))
            C("redistance_full_dev", "redistance_full", lambda d32=d32, g=g: pkg.redistance_full_dev(d32, g))
            C("mesh_distance", "mesh_distance", lambda V=V, T=T, lat=lat, band=band: pkg.mesh_distance(V, T, lat, band, want_index=True, device=0))
            C("mesh_distance_dev", "mesh_distance", lambda dV=dV, dT=dT, lat=lat, band=band: pkg.mesh_distance_dev(dV, dT, lat, band, want_index=True))
            C("mesh_shells", "mesh_shells", lambda V=V, T=T: pkg.mesh_shells(V, T, device=0))
            C("mesh_shells_dev", "mesh_shells", lambda dV=dV, dT=dT: pkg.mesh_shells_dev(dV, dT))
            C("mesh_sections", "mesh_sections", lambda V=V, T=T, levels=levels: pkg.mesh_sections(V, T, (0.0, 0.0, 1.0), levels, device=0))
            C("mesh_sections_dev", "mesh_sections", lambda dV=dV, dT=dT, levels=levels: pkg.mesh_sections_dev(dV, dT, (0.0, 0.0, 1.0), levels))
            C("mesh_weld", "mesh_weld", lambda soup=soup, snap=snap: pkg.mesh_weld(soup, None, snap=snap, device=0))
            C("mesh_weld_dev", "mesh_weld", lambda d_soup=d_soup, snap=snap: pkg.mesh_weld_dev(d_soup, None, snap=snap))
            C("mesh_orient", "mesh_orient", lambda V=V, T=T: pkg.mesh_orient(V, T, outward=True, device=0))
            C("mesh_orient_dev", "mesh_orient", lambda dV=dV, dT=dT: pkg.mesh_orient_dev(dV, dT, outward=True))
            C("mesh_fans", "mesh_fans", lambda V=V, T=T: pkg.mesh_fans(V, T, split=True, device=0))
            C("mesh_fans_dev", "mesh_fans", lambda dV=dV, dT=dT: pkg.mesh_fans_dev(dV, dT, split=True))
            C("mesh_holes", "mesh_holes", lambda V=V, T=T: pkg.mesh_holes(V, T, fill=8, device=0))
            C("mesh_holes_dev", "mesh_holes", lambda dV=dV, dT=dT: pkg.mesh_holes_dev(dV, dT, fill=8))
            C("mesh_intersections", "mesh_intersections", lambda V=V, T=T: pkg.mesh_intersections(V, T, device=0))
            C("mesh_intersections_dev", "mesh_intersections", lambda dV=dV, dT=dT: pkg.mesh_intersections_dev(dV, dT))
            # smoothing: small lattices of its own (a CG solve per call)
            gs = lattice_grid(pkg, ((9, 8, 10), (12, 11, 13), (14, 14, 14))[k])
            r = (2.6, 3.7, 4.6)[k]
            sdf = ball_sdf(gs, r, (0.45 + 0.03 * k, 0.5, 0.52))
            target = 4.0 / 3.0 * np.pi * (r * H) ** 3
            self.smooth_inputs.append((gs, sdf, target))
            C("rbf_smooth", "rbf_smooth", lambda sdf=sdf, gs=gs, target=target, s=1 + k % 2: smoothing(pkg, sdf, gs, s, target))

    def family_list(self, family, t):
        return [c for k in ORDERS[t] for c in self.by_input[family][k]]

    def rounds(self):
        names = list(self.by_input)
        rounds = [Round(f, [self.family_list(f, t) for t in range(N_THREADS)]) for f in names]
        # the mixed round: every thread walks the families in an order of its own, one input each
        mixed = []
        for t in range(N_THREADS):
            order = names[3 * t:] + names[:3 * t]
            if t % 2:
                order = order[::-1]
            mixed.append([c for i, f in enumerate(order) for c in self.by_input[f][(i + t) % 3]])
        return rounds + [Round("mixed", mixed)]

    def check_reference(self, expected):
        import iso_ref
        import mesh_dist_ref64 as M
        from scipy import ndimage
        g, v = self.fields[1]
        nx, ny, nz = g.dims
        lab, _ = ndimage.label(v.astype(np.float64) >= 0.0)
        flat = lab.ravel()
        ids, first = np.unique(flat, return_index=True)
        keep = ids > 0
        roots, sizes = first[keep].astype(np.int64), np.bincount(flat)[ids[keep]].astype(np.int64)
        o = np.argsort(roots)
        got = expected["analyze_components_dev #1"]
        assert len(roots) > 20 and all(np.array_equal(a, b) for a, b in zip(got, (roots[o], sizes[o], roots[o], sizes[o]))), "components vs scipy"
        keys, vals = expected["analyze_components #1"][0::2], expected["analyze_components #1"][1::2]
        assert np.array_equal(np.concatenate(keys), roots[o] + 1) and np.array_equal(np.concatenate(vals), sizes[o]), "components vs scipy"
        dims, origin, spacing = lattice_of(g)
        ref, _ = iso_ref.vertices(v, dims, origin, spacing, 0.0)
        for name in ("extract_isosurface #1", "extract_isosurface_dev #1"):
            assert np.array_equal(expected[name][0].view(np.uint32), ref.view(np.uint32)), name + " vs iso_ref"
        g, _ = self.fields[0]
        V, T = self.meshes[0]
        dims, origin, spacing = lattice_of(g)
        band = 3.0 * spacing
        dr, _ = M.distance_brute(V, T, M.lattice_points(dims, origin, spacing))
        want = np.minimum(dr, band)
        d = expected["mesh_distance #0"][0].ravel()
        assert (np.abs(d - want) <= M.bound(want, M.coord_scale(V, dims, origin, spacing), np.float64)).all(), "mesh_distance vs mesh_dist_ref64"

    def close(self):
        pass


def group_b(pkg):
    fam = Families(pkg)
    return fam.rounds(), fam.check_reference, fam.close


# ---------------------------------------------------------------------------------------------------------------------
# group C: plans on their own streams, host sessions, and the whole pipeline beside other work
# ---------------------------------------------------------------------------------------------------------------------
def plan_runs(pkg, dX, dI, dR, grid):
    """a fresh plan, three runs into poisoned outputs (the first waits for its list sizes, the others speculate) -> the
    three fields and the projection data of the last"""
    import torch
    plan = pkg.DevicePlan(0)
    out = []
    for _ in range(3):
        buf = torch.full((grid.ngp,), float("nan"), dtype=torch.float64, device="cuda:0")
        plan.run(dX, dI, dR, 0.5, grid, sdf=buf)
        out.append(buf)
    d, s = (torch.full((grid.ngp,), float("nan"), dtype=torch.float64, device="cuda:0") for _ in range(2))
    plan.run(dX, dI, dR, 0.5, grid, dist=d, sign=s)
    out += [d, s]
    out = [o.cpu() for o in out]
    plan.close()
    return out


def host_sdf(pkg, mesh, grid, rn):
    st = {}
    dist, xp = pkg.evalDistances(mesh, grid, rn, 0.5, device=0, out=poisoned(grid.ngp), stats=st)
    sign = pkg.Sign_Detection(mesh, grid, rn, 0.5, device=0, out=poisoned(grid.ngp))
    sdf = pkg.sdf_fused(mesh, grid, rn, 0.5, device=0, out=poisoned(grid.ngp))
    return dist, xp, sign, sdf, {k: v for k, v in st.items() if k.startswith("n_")}


def pipeline(pkg, X, IEN, rho):
    info = {}
    opts = pkg.Rho2sdfOptions(sdf_grid_setup="automatic", export_analysis=True)
    fine, fine_grid, grid, dists = pkg.rho2sdf("beam", X, IEN, rho, options=opts, device=0, info=info, surface=True)
    return fine, dists, info["components_before"], info["surface"], info["rho_n"], info["level_shift"], info["n_flipped"], info["cg_iters"]


def group_c(pkg):
    from conftest import load_fixture
    from rho2sdf_jl_amd import synthetic
    Xh, Ih, rh = synthetic.hex_mesh(6, jitter=.30, seed=20240502)
    gh = pkg.Grid(Xh.min(0), Xh.max(0), synthetic.grid_n_max_for_points(40), 3)
    Xt, It, rt = synthetic.tet_mesh(5)
    gt = pkg.Grid(Xt.min(0), Xt.max(0), synthetic.grid_n_max_for_points(32), 3)
    assert max(gh.dims) <= 48 and max(gt.dims) <= 48
    hexd, tetd = [dev(a) for a in (Xh, Ih, rh)], [dev(a) for a in (Xt, It, rt)]
    Xs, Is, rho_s = load_fixture("sphere")
    ms = pkg.Mesh(Xs, Is)
    rs = pkg.DenseInNodes(ms, rho_s, device=0)
    gs = pkg.Grid(Xs.min(0), Xs.max(0), 10, 3)
    X4, I4, r4 = synthetic.hex_mesh(4)
    m4, g4 = pkg.Mesh(X4, I4), pkg.Grid(X4.min(0), X4.max(0), 14, 3)
    plans = Round("two plans, two host callers", [
        [Call("plan hex", "plan", lambda: plan_runs(pkg, *hexd, gh))],
        [Call("plan tet", "plan", lambda: plan_runs(pkg, *tetd, gt))],
        [Call("host sphere", "host", lambda: host_sdf(pkg, ms, gs, rs)), Call("host hex4", "host", lambda: host_sdf(pkg, m4, g4, r4))],
        [Call("host hex4", "host", lambda: host_sdf(pkg, m4, g4, r4)), Call("host sphere", "host", lambda: host_sdf(pkg, ms, gs, rs))]])
    Xb, Ib, rho_b = load_fixture("beam_vfrac_03")
    so, fam = SharedObjects(pkg), Families(pkg)
    smooth = [c for k in (0, 1, 2) for c in fam.by_input["rbf_smooth"][k]]
    tools = [c for f in ("components", "extract", "mesh_shells") for c in fam.by_input[f][1]]
    whole = Round("rho2sdf beside smoothing, a shared field and the tools", [
        [Call("rho2sdf beam", "rho2sdf", lambda: pipeline(pkg, Xb, Ib, rho_b))], smooth, so.lists()[3][:12], tools], repeats=REPEATS)

    def check(expected):
        a, b, c = expected["plan hex"][:3]
        assert differing([a, a], [b, c]) == 0, "the three runs of one plan differ"

    return [plans, whole], check, so.close


# ---------------------------------------------------------------------------------------------------------------------
# group D: the error state belongs to the thread
# ---------------------------------------------------------------------------------------------------------------------
def rejected(pkg, what, fn, outputs):
    """a call that must be refused -> (what, the thread's r2s_last_error, return code); outputs must stay poison"""
    rc = fn()
    msg = pkg._lib.lib().r2s_last_error().decode()
    assert rc != 0, f"{what}: accepted"
    assert all(is_poison(o) for o in outputs), f"{what}: a refused call wrote into an output"
    return what, msg, int(rc)


def group_d(pkg):
    from conftest import load_fixture
    L, lib = pkg._lib, pkg._lib.lib()
    X, IEN, rho = load_fixture("sphere")
    good = pkg.Mesh(X, IEN)
    rn = pkg.DenseInNodes(good, rho, device=0)
    grid = pkg.Grid(X.min(0), X.max(0), 10, 3)
    fl = fields(pkg)
    dp, ip = lambda a: a.ctypes.data_as(L.c_double_p), lambda a: a.ctypes.data_as(L.c_int64_p)   # noqa: E731

    def bad_ien(badval):
        bad = IEN.copy()
        bad[len(bad) // 2, 3] = badval
        out = poisoned(grid.ngp)
        p = pkg.api._params(good, 1.1, 0)

        def fn():
            st = L.R2SStats()
            return lib.r2s_sdf(dp(good.X), good.nnp, ip(bad), good.nel, dp(rn), 0.5, ctypes.byref(grid.c), ctypes.byref(p), dp(out), ctypes.byref(st))
        return lambda: rejected(pkg, f"IEN {badval}", fn, [out])

    def bad_iso(dims, vcap):
        g, v = fl[0]
        _, origin, spacing = pkg.api._iso_lattice(g, None)
        nv, nt = ctypes.c_int64(-1), ctypes.c_int64(-1)
        tris = poisoned(3 * 8, np.int32)
        cd = (ctypes.c_int64 * 3)(*dims)

        def fn():
            return lib.r2s_extract_isosurface(v.ctypes.data_as(ctypes.c_void_p), 1, cd, origin, spacing, 0.0, 0, None, vcap,
                                              tris.ctypes.data_as(L.c_int32_p), 8, ctypes.byref(nv), ctypes.byref(nt))
        return lambda: rejected(pkg, f"isosurface {dims} capacity {vcap}", fn, [tris])

    def valid_sdf(band):
        return lambda: pkg.sdf_fused(good, grid, rn, 0.5, band_factor=band, device=0, out=poisoned(grid.ngp))

    def valid_iso(k):
        return lambda: pkg.extract_isosurface(fl[k][1], fl[k][0], device=0)

    lists = [
        [Call("reject IEN 0", "error", bad_ien(0)), Call("sdf 1.1", "valid", valid_sdf(1.1)),
         Call("reject dims", "error", bad_iso((1, 17, 17), 0)), Call("iso 0", "valid", valid_iso(0))],
        [Call("reject capacity", "error", bad_iso((17, 17, 17), 5)), Call("iso 1", "valid", valid_iso(1)),
         Call("reject IEN nnp+1", "error", bad_ien(len(X) + 1)), Call("sdf 2.5", "valid", valid_sdf(2.5))],
        [Call("sdf 2.5", "valid", valid_sdf(2.5)), Call("iso 2", "valid", valid_iso(2)),
         Call("components 1", "valid", lambda: pkg.analyze_sdf_components(fl[1][1].astype(np.float64).ravel(), fl[1][0], device=0))],
        [Call("iso 0", "valid", valid_iso(0)), Call("sdf 1.1", "valid", valid_sdf(1.1)), Call("iso 1", "valid", valid_iso(1))]]

    def check(expected):
        text = lambda key: bytes(expected[key][1]).decode()   # noqa: E731
        assert "outside 1..nnp" in text("reject IEN 0") and "outside 1..nnp" in text("reject IEN nnp+1")
        assert "every dimension must be >= 2" in text("reject dims")
        assert "null output with capacity > 0" in text("reject capacity")

    return [Round("two rejecting, two valid callers", lists)], check, lambda: None


BUILDERS = {"A": group_a, "B": group_b, "C": group_c, "D": group_d}


# ---------------------------------------------------------------------------------------------------------------------
# the child
# ---------------------------------------------------------------------------------------------------------------------
def main(argv):
    group, out_path = argv[0], argv[1]
    faulthandler.enable()
    faulthandler.dump_traceback_later(HANG_SECONDS, exit=True)   # a deadlock leaves every thread's stack in stderr
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as graft
    t_start = time.perf_counter()
    pkg = graft.load_built()
    import torch
    torch.cuda.set_device(0)
    lib = pkg._lib.lib()
    torch.zeros(1, device="cuda:0")
    lib.r2s_release_cache()
    live_before = int(lib.r2s_live_device_bytes())
    poison_outputs(pkg)
    rounds, check_reference, close = BUILDERS[group](pkg)
    expected = {}
    t_serial = serial_pass(rounds, expected)
    check_reference(expected)
    t_conc, report = concurrent_pass(rounds, expected)
    close()
    del rounds, check_reference, close
    import gc
    gc.collect()
    torch.cuda.synchronize()
    lib.r2s_release_cache()
    live_after = int(lib.r2s_live_device_bytes())
    res = dict(group=group, serial_seconds=round(t_serial, 3), concurrent_seconds=round(t_conc, 3), rounds=report,
               live_before=live_before, live_after=live_after, total_seconds=round(time.perf_counter() - t_start, 2))
    with open(out_path, "w") as f:
        json.dump(res, f)
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main(sys.argv[1:])

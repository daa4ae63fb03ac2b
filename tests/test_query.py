"""Ray queries on the host backend (rtw_trace_rays, rtw_occluded; DESIGN.md §Ray queries): the closest hit and the
occlusion flag of caller-supplied rays against the guide buffers, against the oracle's brute force over every
primitive, under the caller's tmax, across trees (tunings, BVH modes, instance lists and trees, a mesh as an instance
and as world objects), from far origins, with vertex attributes, and with degenerate rays mixed in.  Scenes, ray sets
and cached references: tests/query_scenes.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_scenes as D
import query_scenes as Q
from conftest import REPO

NONE = 0xFFFFFFFF
F = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    """Bit for bit (NaNs and signed zeros included)."""
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def records_equal(a, b, fields=None):
    return all(same(a[f], b[f]) for f in (fields or a.dtype.names))


# ---------------------------------------------------------------- 1. symbols and sizes
def test_symbols_and_struct_sizes(rtw, tmp_path):
    lib, A = rtw.lib(), rtw._abi
    for name in ("rtw_trace_rays", "rtw_trace_rays_device", "rtw_occluded", "rtw_occluded_device"):
        assert hasattr(lib, name), name
    prog = tmp_path / "sizes.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtw_gpu.h"\nint main(){'
                    'printf("%zu %zu %zu %zu %zu %zu %u\\n", sizeof(rtw_ray), sizeof(rtw_hit), offsetof(rtw_ray, dir),'
                    ' offsetof(rtw_hit, p), offsetof(rtw_hit, normal), offsetof(rtw_hit, uv), RTW_HIT_NONE);'
                    'return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [32, 64, 16, 16, 32, 48, NONE]
    assert A.RAY_DTYPE.itemsize == C.sizeof(A.RtwRay) == 32 and A.HIT_DTYPE.itemsize == C.sizeof(A.RtwHit) == 64
    assert [A.HIT_DTYPE.fields[f][1] for f in ("p", "normal", "uv")] == [16, 32, 48] and A.RTW_HIT_NONE == NONE
    for name, (first, words, _) in A.HIT_WORDS.items():
        assert A.HIT_DTYPE.fields[name][1] == 4 * first and A.HIT_DTYPE[name].itemsize == 4 * words
    assert lib.rtw_version() == 8


# ---------------------------------------------------------------- 2. against the guides
@pytest.mark.parametrize("name", Q.GUIDES)
def test_pixel_centre_rays_reproduce_the_guides(rtw, name):
    _, rays = Q.case("guide_" + name)
    hits, _ = Q.host("guide_" + name)
    _, nd = D.host_guides(name)
    hit = hits["kind"] != NONE
    assert np.array_equal(hit, nd[:, 3] > 0) and hit.sum() > 100
    assert same(hits["normal"], nd[:, :3])
    d = rays["dir"]
    len2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    depth = hits["t"] * np.sqrt(len2)
    assert depth.dtype == F and same(depth[hit], nd[hit, 3])
    assert np.isinf(hits["t"][~hit]).all()


def test_rays_see_through_media(rtw):
    smoke, _ = Q.host("guide_cornell_smoke")
    plain, _ = Q.host("guide_cornell_smoke_no_media")
    assert records_equal(smoke, plain, ("t", "p", "normal"))
    hit = smoke["kind"] != NONE                                       # (only the walls are left to hit)
    assert hit.sum() > 400 and (smoke["kind"][hit] == rtw._abi.RTW_OBJ_QUAD).all()


# ---------------------------------------------------------------- 3. against the oracle, brute force
@pytest.mark.parametrize("name", Q.BRUTE)
def test_closest_hit_is_the_oracles_minimum(name):
    hits, _ = Q.host(name)
    t, kind, index, count, _, _ = Q.brute_force(name)
    n = len(t)
    hit = np.isfinite(t)
    tied = hit & (count > 1)
    # what keeps the test honest, on the oracle alone
    assert hit.sum() >= 0.3 * n and (~hit).sum() >= 0.1 * n and tied.sum() <= 0.01 * hit.sum(), \
        (hit.sum(), (~hit).sum(), tied.sum())
    assert same(hits["t"], t)
    once = hit & ~tied
    assert np.array_equal(hits["kind"][once], kind[once]) and np.array_equal(hits["index"][once], index[once])
    assert (hits["kind"][~hit] == NONE).all()
    # top-level primitives: the primitive is the object, no member
    assert np.array_equal(hits["prim_kind"], hits["kind"]) and np.array_equal(hits["prim_index"], hits["index"])
    assert (hits["member"] == NONE).all()


def test_record_fields_of_hits_and_misses(rtw):
    """p = o + t d in fp32 and material = the primitive's, for every hit; the normal is the outward one turned towards
    the ray and front says whether it was turned.  Where fp32 resolves the sphere -- the set's second half (origins
    within 12 of the spheres, |d| < 2) on spheres of radius >= 0.1 -- the normal is unit to 1e-3 and uv lies in
    [0, 1]; a sphere of radius 0.0066 seen from 30 away is below the reference arithmetic's own resolution.  A miss
    is inf, five RTW_HIT_NONE words and ten zero words."""
    _, rays = Q.case("book1_64")
    arr, _ = Q.arrays("book1_64")
    hits, _ = Q.host("book1_64")
    hit = hits["kind"] != NONE
    h, r = hits[hit], rays[hit]
    assert same(h["p"], r["origin"] + h["t"][:, None] * r["dir"])
    assert np.array_equal(h["material"], arr.spheres["material"][h["index"]])
    assert ((h["normal"].astype(np.float64) * r["dir"]).sum(1) <= 0).all()
    outward = h["p"].astype(np.float64) - arr.spheres["center1"][h["index"]]
    assert np.array_equal(h["front"] == 1, (outward * h["normal"]).sum(1) > 0)
    near = (np.nonzero(hit)[0] >= Q.N // 2) & (arr.spheres["radius"][h["index"]] >= 0.1)
    assert near.sum() > 500 and (h["front"][near] == 0).sum() > 5
    assert np.abs(np.linalg.norm(h["normal"][near].astype(np.float64), axis=1) - 1).max() < 1e-3
    assert (h["uv"][near] >= 0).all() and (h["uv"][near] <= 1).all() and h["uv"][near].std() > 0.1
    miss = np.ascontiguousarray(hits[~hit]).view(np.uint32).reshape(-1, 16)
    want = np.zeros(16, np.uint32)
    want[0] = bits(np.array([np.inf], F))[0]
    want[[1, 2, 3, 14, 15]] = NONE
    assert len(miss) > 400 and (miss == want).all()


# ---------------------------------------------------------------- 4. tmax
@pytest.mark.parametrize("name", Q.TMAX_BASES)
def test_tmax_is_an_open_bound(name):
    hits, _ = Q.host(name)
    found = hits[hits["kind"] != NONE]
    assert len(found) > 1000
    at, occ_at = Q.host("tmax_eq_" + name)          # tmax = t*: nothing closer exists, and t* itself is excluded
    assert (at["kind"] == NONE).all() and np.isinf(at["t"]).all() and not occ_at.any()
    nxt, occ_next = Q.host("tmax_next_" + name)      # tmax = nextafter(t*): the identical record
    assert records_equal(nxt, found) and occ_next.all()


def test_empty_intervals_miss():
    hits, occ = Q.host("tmax_bad")                   # tmax = NaN, 0, 0.001
    assert (hits["kind"] == NONE).all() and np.isinf(hits["t"]).all() and not occ.any()
    full, _ = Q.host("book1_64")
    assert (full["kind"][:768] != NONE).sum() > 200  # (the same rays do hit when unbounded or bounded further out)


# ---------------------------------------------------------------- 5. occlusion
@pytest.mark.parametrize("name", [c for c in Q.CASES if c != "degenerate"])   # (unspecified records there)
def test_occluded_is_trace_hit(name):
    hits, occ = Q.host(name)
    assert occ.dtype == bool and np.array_equal(occ, hits["kind"] != NONE)


# ---------------------------------------------------------------- 6. tree independence
def test_book1_trees_agree():
    base, _ = Q.host("book1")
    assert (base["kind"] != NONE).sum() > 1500
    for other in Q.TREE_BOOK1[1:]:
        assert records_equal(Q.host(other)[0], base, ("t", "index", "p", "normal")), other


def test_cornell_lists_and_instance_trees_agree(rtw):
    lst, _ = Q.host("cornell_list")
    tree, _ = Q.host("cornell_tree")
    assert records_equal(lst, tree)
    inst = lst[lst["kind"] == rtw._abi.RTW_OBJ_INSTANCE]
    assert len(inst) > 300 and (inst["member"] < 6).all() and (inst["prim_kind"] == rtw._abi.RTW_OBJ_QUAD).all()
    arr, _ = Q.arrays("cornell_list")
    ref = arr.members[arr.instances["first"][inst["index"]] + inst["member"]]
    assert np.array_equal(ref["kind"], inst["prim_kind"]) and np.array_equal(ref["index"], inst["prim_index"])
    assert np.array_equal(inst["material"], arr.quads["material"][inst["prim_index"]])


def test_mesh_as_instance_and_as_world_objects_agree(rtw):
    inst, _ = Q.host("mesh_inst")
    top, _ = Q.host("mesh_top")
    arr, _ = Q.arrays("mesh_inst")
    assert len(arr.instances) == 1 and arr.instances["count"][0] == 320 > rtw._abi.RTW_INST_LIST_MAX
    rest = [f for f in inst.dtype.names if f not in ("kind", "index", "member")]
    assert records_equal(inst, top, rest)
    hit = inst["kind"] != NONE
    assert hit.sum() > 1500 and (inst["kind"][hit] == rtw._abi.RTW_OBJ_INSTANCE).all() and (inst["index"][hit] == 0).all()
    assert np.array_equal(inst["member"][hit], inst["prim_index"][hit])
    assert (top["kind"][hit] == rtw._abi.RTW_OBJ_QUAD).all() and np.array_equal(top["index"], top["prim_index"])


# ---------------------------------------------------------------- 7. far origins
def test_far_origins_book1_against_the_oracle():
    """From 100 x extent the walk takes the reference's box arithmetic per ray, and the closest hit is the oracle's
    brute-force minimum, t bit for bit -- with the ground hoisted (the default) and with the ground under the tree's
    boxes (hoist 0), where a box test from 2e5 out decides whether it is reached.

    The rays are those of 8192 seeded candidates that fp32 resolves (query_scenes.resolved: decided from the geometry
    in float64, before any trace).  Book-1's extent is 2000 (the ground sphere), so the origins lie 2e5 out:
    Sphere.hit's discriminant then carries a rounding of 5e-7 of its terms, and a ray passing within some 140 units
    of a small sphere cannot be told from one that hits it.  A brute force over such rays reports spheres up to 80
    units in front of their targets (aimed at the primitive centres, it differs in t from this walk on 520 of 1024
    rays and from the reference's own tree, RTW_BVH_REFERENCE, on 515): it is a reference only where it is resolved.
    What is left hits the ground sphere away from the field, or misses."""
    _, rays = Q.case("far_book1")
    assert len(rays) == 1024 and np.abs(rays["origin"]).max(1).min() > 7 * Q.extent_of("book1_64")
    t, kind, index, count, _, _ = Q.brute_force("far_book1")
    hit = np.isfinite(t)
    assert hit.sum() >= 0.3 * len(t) and (~hit).sum() >= 0.1 * len(t) and (count[hit] == 1).all(), (hit.sum(), (~hit).sum())
    for name in ("far_book1", "far_book1_hoist0"):
        w = Q.world(Q.case(name)[0])
        assert w.stats()["n_hoisted"] == (0 if name.endswith("hoist0") else 1)
        w.close()
        hits, occ = Q.host(name)
        assert same(hits["t"], t), name
        assert np.array_equal(hits["kind"], kind) and np.array_equal(hits["index"], index), name
        assert np.array_equal(occ, hit), name


def test_far_origins_cornell_against_near_origins():
    """The same rays started 1000 units before their targets (inside 7 x extent: the FMA slab test) hit the same
    primitive on the same side at the same point.  p within 1e-4 of its length: an origin 5.5e4 out carries an fp32
    rounding of 2e-3 per coordinate, o + t d as much again, against |p| of 1e2 .. 1e3."""
    _, far_r = Q.case("far_cornell")
    _, near_r = Q.case("near_cornell")
    ext = Q.extent_of("cornell")
    assert np.abs(far_r["origin"]).max(1).min() > 7 * ext > np.abs(near_r["origin"]).max()
    far, _ = Q.host("far_cornell")
    near, _ = Q.host("near_cornell")
    hit = near["kind"] != NONE
    assert hit.sum() > 900
    for f in ("kind", "index", "member", "prim_kind", "prim_index", "front"):
        assert np.array_equal(far[f], near[f]), f
    dp = np.abs(far["p"][hit].astype(np.float64) - near["p"][hit]).max(1)
    assert (dp <= 1e-4 * np.linalg.norm(near["p"][hit].astype(np.float64), axis=1)).all(), dp.max()


# ---------------------------------------------------------------- 8. attributes
def test_smooth_triangles_carry_the_attribute_record(rtw):
    """Hits on the smooth icosphere of cornell_mesh: normal, uv and front are rtw_debug_quad_shade's for the same
    (quad, object-space ray, t), the normal taken back to the world."""
    import smooth_scenes as S
    A = rtw._abi
    _, rays = Q.case("attr_cornell_mesh")
    arr, _ = Q.arrays("cornell_mesh")
    hits, _ = Q.host("attr_cornell_mesh")
    quads, attrs = arr.vertex_attrs
    assert len(quads) == 320
    ball = np.nonzero((hits["kind"] == A.RTW_OBJ_INSTANCE) & np.isin(hits["prim_index"], quads))[0]
    assert len(ball) > 300
    h = hits[ball]
    assert (h["prim_kind"] == A.RTW_OBJ_QUAD).all()
    oo, od, to_world = Q.ball_object_space(rays[ball])
    by_quad = np.zeros(len(arr.quads), A.VERTEX_ATTR_DT)
    by_quad[quads] = attrs
    nrm, uv, front = S.quad_shade(rtw, arr.quads[h["prim_index"]], by_quad[h["prim_index"]], oo, od, h["t"])
    assert same(h["normal"], to_world(nrm)) and same(h["uv"], uv) and np.array_equal(h["front"] == 1, front)
    # and they are shading normals: the flat scene's differ
    flat = Q.host("flat_cornell_mesh")[0][ball]
    assert same(flat["t"], h["t"]) and (bits(flat["normal"]) != bits(h["normal"])).any(1).mean() > 0.9


# ---------------------------------------------------------------- 9. degenerate rays, refusals, independence
def test_nothing_to_do_and_refusals(rtw):
    A, L = rtw._abi, rtw.lib()
    w = Q.world("book1_64")
    _, rays = Q.case("book1_64")
    r = rays[:8].copy()
    hits = np.full(8, 7, np.uint8).repeat(64).view(A.HIT_DTYPE)
    occ = np.full(8, 7, np.uint8)
    before = hits.copy()
    assert L.rtw_trace_rays(w.handle, 0, r.ctypes.data, hits.ctypes.data) == A.RTW_OK
    assert L.rtw_occluded(w.handle, 0, r.ctypes.data, occ.ctypes.data) == A.RTW_OK
    assert L.rtw_trace_rays(w.handle, 0, None, None) == A.RTW_OK and L.rtw_occluded(w.handle, 0, None, None) == A.RTW_OK
    for rc in (L.rtw_trace_rays(w.handle, 8, None, hits.ctypes.data), L.rtw_trace_rays(w.handle, 8, r.ctypes.data, None),
               L.rtw_occluded(w.handle, 8, None, occ.ctypes.data), L.rtw_occluded(w.handle, 8, r.ctypes.data, None),
               L.rtw_trace_rays(None, 8, r.ctypes.data, hits.ctypes.data),
               L.rtw_occluded(None, 8, r.ctypes.data, occ.ctypes.data),
               L.rtw_trace_rays(w.handle, 1 << 32, r.ctypes.data, hits.ctypes.data),
               L.rtw_occluded(w.handle, 1 << 32, r.ctypes.data, occ.ctypes.data),
               L.rtw_trace_rays_device(w.handle, 8, r.ctypes.data, hits.ctypes.data, None, 0),   # a host context
               L.rtw_occluded_device(w.handle, 8, r.ctypes.data, occ.ctypes.data, None, 0)):
        assert rc == A.RTW_E_INVALID
        assert L.rtw_last_error()
    assert same(hits.view(np.uint32), before.view(np.uint32)) and (occ == 7).all()
    assert len(w.trace(np.zeros((0, 3)), np.zeros((0, 3)))) == 0 and len(w.occluded(rays[:0])) == 0
    w.close()


def test_degenerate_rays_leave_the_others_alone():
    _, rays = Q.case("book1_64")
    mixed, bad = Q.degenerate(rays[:1024])
    assert bad.sum() == 64 and same(mixed["dir"], Q.case("degenerate")[1]["dir"])
    clean, clean_occ = Q.host("book1_64")
    got, occ = Q.host("degenerate")                                        # (the call returned)
    assert records_equal(got[~bad], clean[:1024][~bad]) and np.array_equal(occ[~bad], clean_occ[:1024][~bad])


def test_permuted_rays_give_permuted_records():
    _, rays = Q.case("cornell_tree")
    hits, occ = Q.host("cornell_tree")
    perm = np.random.default_rng(3).permutation(len(rays))
    assert same(Q.case("permuted_cornell_tree")[1]["origin"], rays["origin"][perm])
    got, got_occ = Q.host("permuted_cornell_tree")
    w = Q.world("cornell_tree")
    one = w.trace(rays["origin"][17], rays["dir"][17], tmax=rays["tmax"][17], time=rays["time"][17])
    w.close()
    assert records_equal(got, hits[perm]) and np.array_equal(got_occ, occ[perm])
    assert len(one) == 1 and records_equal(one, hits[17:18])


def test_host_buffers_need_no_16_byte_alignment(rtw):
    """rtw_ray / rtw_hit have the alignment of a float: a C caller's array may start on any multiple of 4."""
    _, rays = Q.case("cornell_tree")
    want, want_occ = Q.host("cornell_tree")
    n = 300
    raw_in = np.zeros(32 * n + 16, np.uint8)
    raw_out = np.zeros(64 * n + 16, np.uint8)
    base_in = raw_in.ctypes.data + (-raw_in.ctypes.data) % 16 + 4
    base_out = raw_out.ctypes.data + (-raw_out.ctypes.data) % 16 + 4
    r = np.frombuffer(raw_in, np.uint8, 32 * n, base_in - raw_in.ctypes.data)
    r[:] = rays[:n].view(np.uint8)
    occ = np.zeros(n + 1, np.uint8)
    w = Q.world("cornell_tree")
    rtw._abi.check(rtw.lib().rtw_trace_rays(w.handle, n, base_in, base_out), "rtw_trace_rays")
    rtw._abi.check(rtw.lib().rtw_occluded(w.handle, n, base_in, occ.ctypes.data + 1), "rtw_occluded")
    w.close()
    got = np.frombuffer(raw_out, np.uint8, 64 * n, base_out - raw_out.ctypes.data).copy().view(rtw._abi.HIT_DTYPE)
    assert base_in % 16 == 4 and base_out % 16 == 4
    assert records_equal(got, want[:n]) and np.array_equal(occ[1:] == 1, want_occ[:n])

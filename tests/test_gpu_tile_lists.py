"""The camera-ray candidate lists as the GPU builds them (wf_tile_lists: the flat scan; wf_tile_lists_walk: the
frustum walk), read back through rtw_debug_tile_lists and held against the float64 reference of tests/tile_scenes.py:
every slot written, distinct leaves with the nodes' own centre and r^2, sorted by (tlow, id), a superset of what
brute-force rays hit with tlow below the first hit, between the documented bound without margins (R0) and with the
margins doubled (R2), and given up (RTW_TL_WALK) only when there are more candidates than the cap.  Then the cap's
edges, and the images at caps on both sides of 64 (the scan's block has 64 lanes for up to 128 candidates)."""
import ctypes as C

import numpy as np
import pytest

import tile_scenes as TS

pytestmark = pytest.mark.gpu

GPU = 0
BUILDERS = {1: "scan", 2: "walk"}


@pytest.fixture(scope="module")
def worlds(rtw):
    import torch
    assert torch.cuda.is_available()
    made = {s: rtw.World(TS.arrays(s), device=GPU) for s in ("book1", "stress")}
    yield made
    for w in made.values():
        w.close()


def same_bits(a, b):
    """Two readbacks equal word for word (unwritten float slots are NaN patterns)."""
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a[:5], b[:5])) and a[5:] == b[5:]


def lists(world, cam_name, builder, cap=128):
    cam, a, b = TS.camera(cam_name)
    return world.debug_tile_lists(cam, a, b, builder=builder, cap=cap)


def test_tree_sizes_pick_both_builders(rtw, worlds):
    """Book-1's tree is a small one (the render scans), the stress world's is above 4096 nodes (the render walks), and
    builder 0 is that choice: the same lists as the builder named."""
    small, large = worlds["book1"].stats()["n_nodes"], worlds["stress"].stats()["n_nodes"]
    assert small <= 4096 < large, (small, large)
    for scene, same in (("book1", 1), ("stress", 2)):
        auto, named = lists(worlds[scene], "i", 0), lists(worlds[scene], "i", same)
        assert same_bits(auto, named)
    # the universe the reference used is this context's tree
    for scene in worlds:
        ids, centres, radii = TS.universe(worlds[scene].nodes())
        ref = TS.reference(scene, "i", GPU)
        assert np.array_equal(ids, ref["ids"]) and np.array_equal(centres, ref["centres"])


@pytest.mark.parametrize("builder", sorted(BUILDERS), ids=BUILDERS.get)
@pytest.mark.parametrize("cam_name", sorted(TS.CAMERAS))
@pytest.mark.parametrize("scene", ["book1", "stress"])
def test_lists_against_reference(rtw, worlds, scene, cam_name, builder):
    """Either builder at cap 128 on a small tree (Book-1, 485 spheres) and on one above 4096 nodes (3000 spheres), for
    the cameras of tile_scenes.CAMERAS: every tile that is not RTW_TL_WALK passes checks 1-6 below, and a tile is
    RTW_TL_WALK only if R2 holds more than 128 spheres and always if R0 does (7).  Prints the band counts and how far
    the lists are from R0 and R2."""
    ref = TS.reference(scene, cam_name, GPU)
    counts, ids, tlow, centres, rr, n_tx, row0 = lists(worlds[scene], cam_name, builder)
    assert (n_tx, row0, len(counts)) == (ref["n_tx"], ref["row0"], ref["n_tiles"])
    index = np.full(int(ref["ids"].max()) + 1, -1, np.int64)  # node index -> position in the universe
    index[ref["ids"]] = np.arange(len(ref["ids"]))
    excess = spare = more = fewer = 0  # (figures for profiles/tile_lists/README.md)
    for t in range(ref["n_tiles"]):
        n0, n2 = int(ref["R0"][t].sum()), int(ref["R2"][t].sum())
        # 7. given up only above the cap
        if counts[t] == TS.TL_WALK:
            assert n2 > TS.TL_MAX, (t, n0, n2)
            continue
        assert n0 <= TS.TL_MAX and counts[t] <= TS.TL_MAX, (t, n0, counts[t])
        n = int(counts[t])
        if np.isnan(ref["bounds"][t][0]):
            assert n == 0, (t, n)  # no pixel of the tile is rendered
        # 1. every slot was written; nothing past the count was
        assert (ids[t, :n] != 0xFFFFFFFF).all(), (t, n, np.flatnonzero(ids[t, :n] == 0xFFFFFFFF))
        assert (ids[t, n:] == 0xFFFFFFFF).all(), t
        # 2. distinct leaves
        assert len(np.unique(ids[t, :n])) == n and (ids[t, :n] <= ref["ids"].max()).all(), t
        pos = index[ids[t, :n]]
        assert (pos >= 0).all(), t
        # 3. the node's centre and fl(r * r), bit for bit
        assert np.array_equal(centres[t, :n].view(np.uint32), ref["centres"][pos].view(np.uint32)), t
        assert np.array_equal(rr[t, :n].view(np.uint32), (ref["radii"][pos] * ref["radii"][pos]).view(np.uint32)), t
        # 4. sorted by (tlow, id)
        tl = tlow[t, :n]
        assert (np.diff(tl) >= 0).all(), t
        assert (np.diff(ids[t, :n].astype(np.int64))[np.diff(tl) == 0] > 0).all(), t
        # 5. a superset of what the rays hit, each bound below its first hit
        member = np.zeros(len(ref["ids"]), bool)
        member[pos] = True
        hit = np.isfinite(ref["t_min"][t])
        assert not (hit & ~member).any(), (t, ref["ids"][hit & ~member])
        bound = np.full(len(ref["ids"]), np.inf)
        bound[pos] = tl
        assert (bound[hit] <= ref["t_min"][t][hit]).all(), (t, ref["ids"][hit & (bound > ref["t_min"][t])])
        # 6. between the bound without margins and with twice the code's
        assert not (member & ~ref["R2"][t]).any(), (t, ref["ids"][member & ~ref["R2"][t]])
        if builder == 1:
            assert not (ref["R0"][t] & ~member).any(), (t, ref["ids"][ref["R0"][t] & ~member])
        assert (ref["tlow2"][t][pos] <= tl).all() and (tl <= ref["tlow0"][t][pos]).all(), t
        excess, spare = max(excess, n - n0), max(spare, n2 - n)
        # against the float64 restatement at the code's own margins: an entry beyond it is an entry nearer to R2's
        # edge than the code's margin, a member of it left out one nearer to R0's (or pruned by the walk)
        more, fewer = more + int((member & ~ref["R1"][t]).sum()), fewer + int((ref["R1"][t] & ~member).sum())
    print(f"{scene} {cam_name} {BUILDERS[builder]}: tiles by |R0| (0, 1..32, 33..64, 65..128, >128) = {TS.bands(ref)}; "
          f"walked {int((counts == TS.TL_WALK).sum())}; max |list| - |R0| = {excess}; max |R2| - |list| = {spare}; "
          f"entries outside / spheres left out of the float64 twin at the code's margins = {more} / {fewer}")


def test_cameras_cover_every_band(rtw):
    """The coverage the cases above rest on, from the reference's own counts over the cameras on Book-1: lists on both
    sides of the 64 lanes of the scan's block, tiles above the cap, and empty tiles."""
    total = np.zeros(5, int)
    for cam_name in sorted(TS.CAMERAS):
        b = TS.bands(TS.reference("book1", cam_name, GPU))
        print(f"book1 {cam_name}: tiles by |R0| (0, 1..32, 33..64, 65..128, >128) = {b}")
        total += b
    empty, _, mid, high, over = total
    assert high >= 2 and mid >= 2 and over >= 1 and empty >= 1, total


@pytest.mark.parametrize("builder", sorted(BUILDERS), ids=BUILDERS.get)
@pytest.mark.parametrize("cap", [2, 32, 63, 64, 65, 127, 128])
def test_cap_edges(rtw, worlds, builder, cap):
    """Camera (i) on Book-1 at a cap: a tile whose cap-128 list fits has exactly that list, entry for entry and bit
    for bit; a tile with more candidates walks the tree."""
    full = lists(worlds["book1"], "i", builder, 128)
    got = lists(worlds["book1"], "i", builder, cap)
    assert got[1].shape[1] == cap
    n128 = full[0]
    fits = (n128 != TS.TL_WALK) & (n128 <= cap)
    assert np.array_equal(got[0][fits], n128[fits]) and (got[0][~fits] == TS.TL_WALK).all()
    assert fits.any() and (~fits).any()
    for t in np.flatnonzero(fits):
        n = int(n128[t])
        for x, y in zip(got[1:5], full[1:5]):
            assert np.array_equal(x[t, :n].view(np.uint32), y[t, :n].view(np.uint32)), (t, n)


def test_hook_refuses_what_has_no_lists(rtw, worlds):
    """RTW_E_INVALID: a host context, a world with tile_lists 0, a world of objects (the Cornell box), bad arguments."""
    cam = TS.camera("i")[0]
    host = rtw.World(TS.arrays("book1"), device=TS.CPU)
    off = rtw.World(TS.arrays("book1"), device=GPU, tuning={"tile_lists": 0})
    objects = rtw.World(rtw.flatten(rtw.worlds.cornell_box()), device=GPU)
    try:
        for w in (host, off, objects):
            with pytest.raises(rtw.RtwError) as e:
                w.debug_tile_lists(cam)
            assert e.value.code == rtw._abi.RTW_E_INVALID
        for kw in (dict(builder=3), dict(cap=1), dict(cap=129)):
            with pytest.raises(rtw.RtwError) as e:
                worlds["book1"].debug_tile_lists(cam, **kw)
            assert e.value.code == rtw._abi.RTW_E_INVALID
        # tiles_cap too small: the tile count is still reported
        n, n_tx, row0 = C.c_uint32(), C.c_uint32(), C.c_uint32()
        rc = rtw.lib().rtw_debug_tile_lists(worlds["book1"].handle, C.byref(cam.derived), 0, cam.size, 0, 0, C.byref(n),
                                            C.byref(n_tx), C.byref(row0), None, None, 0)
        assert rc == rtw._abi.RTW_E_INVALID and (n.value, n_tx.value, row0.value) == (15, 5, 0)
        # the world's own cap (32 for a small tree): the packed (tiles, 32) form
        own = worlds["book1"].debug_tile_lists(cam)
        assert own[1].shape == (15, 32)
        full = lists(worlds["book1"], "i", 1, 32)
        assert same_bits(own, full)
    finally:
        for w in (host, off, objects):
            w.close()


# ---------------------------------------------------------------- images
def _render(rtw, world, cam, seed=3):
    import torch
    acc = torch.zeros((cam.size, 4), dtype=torch.float32, device="cuda")
    rc = rtw.lib().rtw_render_device(world.handle, C.byref(cam.derived), 0, cam.size, 0, cam.samples_per_pixel, seed,
                                     acc.data_ptr(), None, None)
    rtw._abi.check(rc, "rtw_render_device")
    return acc.cpu().numpy()


@pytest.mark.parametrize("scene,caps", [("book1", (0, 32, 64, 65, 96, 128)), ("stress", (0, 64, 128))])
@pytest.mark.parametrize("cam_name", ["i", "iv"])
def test_images_do_not_depend_on_the_cap(rtw, scene, cam_name, caps):
    """spp 4, max_depth 8: every cap renders the bits of the walk (tile_lists 0), on both sides of 64."""
    cam = TS.camera(cam_name)[0]
    outs = []
    for cap in caps:
        w = rtw.World(TS.arrays(scene), device=GPU, tuning={"tile_lists": cap})
        outs.append(_render(rtw, w, cam))
        w.close()
    assert np.isfinite(outs[0]).all() and (outs[0][:, 3] == cam.samples_per_pixel).all()
    for cap, out in zip(caps[1:], outs[1:]):
        assert np.array_equal(out, outs[0]), (cap, int((out != outs[0]).any(axis=1).sum()))

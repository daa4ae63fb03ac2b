"""Per-instance BVH (RTW_INST_BVH; every instance of more than 127 members): the tree the library builds, and
the host backend's renders through it against the oracle -- whose HittableList.hit has no member cap -- and
against the member loop.  CPU only.

Bounds are the project's: host backend vs oracle 1e-5 * max(1, |ref|) per channel (tests/test_cpu_backend.py),
5e-5 for the deep / textured final scene (tests/test_gpu_objects.py REL).  Tree vs list is bit for bit."""
import ctypes as C

import numpy as np
import pytest

import instance_tree_scenes as S

CPU = S.CPU
# rtw_scene_hash of two scenes without instance trees, as the library computed it before the feature
HASH_BEFORE = {"cornell": 0xB8FE289DF2F07662, "cornell_smoke": 0x8101F118AEA7F9B0}


def _u32(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _true_boxes(arr, inst):
    """Object-space bounds of every member: spheres span both centres, quads all four corners."""
    lo, hi = [], []
    for m in arr.members[inst["first"]:inst["first"] + inst["count"]]:
        if m["kind"] == 0:
            s = arr.spheres[m["index"]]
            cs = [s["center1"]] + ([s["center2"]] if s["is_moving"] else [])
            lo.append(np.min([c - s["radius"] for c in cs], axis=0))
            hi.append(np.max([c + s["radius"] for c in cs], axis=0))
        else:
            q = arr.quads[m["index"]]
            pts = [q["q"], q["q"] + q["u"], q["q"] + q["v"], q["q"] + q["u"] + q["v"]]
            lo.append(np.min(pts, axis=0))
            hi.append(np.max(pts, axis=0))
    return np.array(lo), np.array(hi)


def _check_tree(arr, i, nodes):
    inst = arr.instances[i]
    count = int(inst["count"])
    n = len(nodes)
    assert n == 2 * count - 1
    w = _u32(nodes["a"][:, 3])
    leaf = (w & 0x80000000) != 0
    skip = (w & 0x7FFFFFFF).astype(np.int64)
    member = _u32(nodes["b"][:, 1])
    assert sorted(member[leaf].tolist()) == list(range(count))          # every member in exactly one leaf
    lo, hi = _true_boxes(arr, inst)
    for j in range(n):
        assert j < skip[j] <= n                                          # in range
        if leaf[j]:
            assert skip[j] == j + 1
            ref = arr.members[inst["first"] + member[j]]
            assert _u32(nodes["b"][j, 2]) == ref["index"]
            assert (_u32(nodes["b"][j, 3]) >> 8) & 0xFF == ref["kind"]
            if ref["kind"] == 0:                                         # the sphere inline
                s = arr.spheres[ref["index"]]
                assert np.array_equal(nodes["a"][j, :3], s["center1"]) and nodes["b"][j, 0] == s["radius"]
                assert (_u32(nodes["b"][j, 3]) & 1) == s["is_moving"]
            continue
        assert (skip[j + 1:skip[j]] <= skip[j]).all()                    # nested
        c2 = skip[j + 1]                                                 # binary: two children fill the subtree
        assert c2 < skip[j] and skip[c2] == skip[j]
        below = member[j + 1:skip[j]][leaf[j + 1:skip[j]]]
        assert (nodes["a"][j, :3] <= lo[below]).all() and (nodes["b"][j, :3] >= hi[below]).all()


@pytest.mark.parametrize("count", [128, 300])
def test_large_instances_accepted_with_valid_tree(rtw, count):
    """Refused before this feature (more than 127 members).  One member moves; one is a skewed quad."""
    rng = np.random.default_rng(count)
    mat = rtw.Lambertian.fromColor([0.5, 0.5, 0.5])
    big = rtw.HittableList.init()
    for k, c in enumerate((rng.random((count, 3)) * 100).astype(np.float32)):
        if k == 3:
            big.add(rtw.Sphere.initMoving(c, c + np.array([40, -30, 25], np.float32), 4, mat))
        elif k == 9:
            big.add(rtw.Quad.init(c, [10, 3, 0], [2, 12, 5], mat))
        else:
            big.add(rtw.Sphere.init(c, 4, mat))
    small = rtw.createBox([0, 0, 0], [10, 10, 10], mat)
    arr = rtw.flatten([rtw.Translate.init(rtw.RotateY.init(big, 20), [5, 6, 7]), rtw.Translate.init(small, [300, 0, 0]),
                       rtw.Sphere.init([0, -1000, 0], 1000, mat)])
    assert arr.instances[0]["flags"] == rtw._abi.RTW_INST_LIST | rtw._abi.RTW_INST_BVH
    assert arr.instances[1]["flags"] == rtw._abi.RTW_INST_LIST
    arr.instances["flags"][0] = rtw._abi.RTW_INST_LIST            # above 127 members: a tree, flagged or not
    for mode in ("sah", "reference"):
        arr.bvh_mode = S.mode_of(rtw, mode)
        world = rtw.World(arr, device=CPU)
        _check_tree(arr, 0, world.instance_nodes(0))
        assert len(world.instance_nodes(1)) == 0                  # an unflagged 6-member instance: no tree
        with pytest.raises(rtw.RtwError):
            world.instance_nodes(2)
        world.close()


@pytest.mark.parametrize("mode", ["sah", "reference"])
def test_cluster_vs_oracle(rtw, mode):
    got = S.host_image("cluster", mode)
    ref = S.oracle_image("cluster")
    assert np.isfinite(got).all() and (got[:, 3] == S.SPP).all()
    ok = S.close(got[:, :3], ref[:, :3], 1e-5)
    assert ok.all(), (ok.mean(), np.abs(got[:, :3] - ref[:, :3]).max())


def test_medium_bounded_by_tree_instance_vs_oracle(rtw):
    got = S.host_image("medium")
    ref = S.oracle_image("medium")
    assert np.isfinite(got).all() and (got[:, 3] == S.SPP).all()
    ok = S.close(got[:, :3], ref[:, :3], 1e-5)
    assert ok.all(), (ok.mean(), np.abs(got[:, :3] - ref[:, :3]).max())
    assert not np.array_equal(got[:, :3], np.broadcast_to(got[0, :3], got[:, :3].shape))


@pytest.mark.parametrize("pair", [("cornell_tree", "cornell_list"), ("rot12_tree", "rot12_list"),
                                  ("cluster", "cluster3")])
@pytest.mark.parametrize("mode", ["sah", "reference"])
def test_tree_equals_list_on_host(rtw, pair, mode):
    """The tree accelerates the list and changes no hit: identical images, exact quad ties included."""
    assert np.array_equal(S.host_image(pair[0], mode), S.host_image(pair[1], mode))


def test_flag_really_builds_trees(rtw):
    for name, want in (("cornell_tree", [11, 11]), ("cornell_list", [0, 0]), ("rot12_tree", [23]), ("rot12_list", [0]),
                       ("cluster", [599]), ("cluster3", [0, 0, 0])):
        world = rtw.World(S.arrays(rtw, name), device=CPU)
        assert [len(world.instance_nodes(i)) for i in range(len(want))] == want, name
        world.close()


def test_scenes_without_trees_keep_hash_and_nodes(rtw):
    """Unflagged scenes keep their scene image (rtw_scene_hash) byte for byte; the flag does not change the
    world tree (the instance's reference box is the list's), only the instance records, which name their trees."""
    L = rtw.lib()

    def ident(arr):
        world = rtw.World(arr, device=CPU)
        h = C.c_uint64()
        rtw._abi.check(L.rtw_scene_hash(world.handle, C.byref(h)), "rtw_scene_hash")
        nodes = world.nodes().tobytes()
        world.close()
        return h.value, nodes

    plain, flagged = ident(S.arrays(rtw, "cornell_list")), ident(S.arrays(rtw, "cornell_tree"))
    assert plain[1] == flagged[1]            # same world tree: the flag does not change the instance's box
    assert plain[0] != flagged[0]            # the instance records name their trees
    # scenes without trees keep the scene image they had before instance trees existed: these are the hashes
    # the library gave before the feature (SAH; Cornell box, Cornell smoke)
    assert plain[0] == HASH_BEFORE["cornell"]
    assert ident(rtw.flatten(rtw.worlds.cornell_smoke()))[0] == HASH_BEFORE["cornell_smoke"]


def test_reduced_final_scene_vs_oracle(rtw):
    ref = S.oracle_image("final")
    got = S.host_image("final", "reference")
    assert np.isfinite(got).all() and (got[:, 3] == S.SPP).all()
    ok = S.close(got[:, :3], ref[:, :3], 5e-5)
    assert ok.all(), (ok.mean(), np.abs(got[:, :3] - ref[:, :3]).max())
    sah = S.host_image("final", "sah")
    ok = S.close(sah[:, :3], ref[:, :3], 5e-5).all(axis=1)
    assert ok.mean() >= 0.999, ok.mean()     # topology-dependent quad ties (adjacent ground boxes)


def _raw_scene(rtw, n_world, n_members):
    """n_world world spheres and one instance of n_members spheres, built as arrays."""
    A = rtw._abi
    n = n_world + n_members
    sph = np.zeros(n, A.SPHERE_DT)
    sph["center1"] = (np.random.default_rng(0).random((n, 3)) * 1000).astype(np.float32)
    sph["radius"] = 1
    mats = np.zeros(1, A.MATERIAL_DT)
    texs = np.zeros(1, A.TEXTURE_DT)
    members = np.zeros(n_members, A.OBJECT_DT)
    members["index"] = np.arange(n_world, n)
    inst = np.zeros(1, A.INSTANCE_DT)
    inst["count"], inst["flags"] = n_members, A.RTW_INST_LIST
    objs = np.zeros(n_world + 1, A.OBJECT_DT)
    objs["index"][:n_world] = np.arange(n_world)
    objs["kind"][n_world] = A.RTW_OBJ_INSTANCE
    return rtw.SceneArrays(sph, mats, texs, np.zeros(0, A.PERLIN_DT), [], members=members, instances=inst, objects=objs)


def test_refusals(rtw):
    arr = _raw_scene(rtw, 4, 200)
    rtw.World(arr, device=CPU).close()
    arr.instances["count"] = 201                                  # first + count past the members
    with pytest.raises(rtw.RtwError):
        rtw.World(arr, device=CPU)
    arr.instances["count"], arr.instances["first"] = 200, 1
    with pytest.raises(rtw.RtwError):
        rtw.World(arr, device=CPU)
    # 16385 world leaves -> at least 16385 nodes (15 bits or more) and 131072 members (17 bits): more than the
    # 31 bits of a hit id
    with pytest.raises(rtw.RtwError, match="hit id limit.*31 bits"):
        rtw.World(_raw_scene(rtw, 16384, 131072), device=CPU)
    rtw.World(_raw_scene(rtw, 16383, 65536), device=CPU).close()  # at most 32767 nodes (15 bits) + 16 bits: fits

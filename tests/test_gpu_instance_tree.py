"""Per-instance BVH on the GPU (inst_tree_t in the RTW_F_ALL | RTW_F_TREE kernels): against the oracle
(5e-5, tests/test_gpu_objects.py REL), bit for bit against the host backend, across the kernel families and
their tunings, and bit for bit against the member loop.  Scenes and references: tests/instance_tree_scenes.py."""
import numpy as np
import pytest

import instance_tree_scenes as S

pytestmark = pytest.mark.gpu

REL = 5e-5


def gpu_image(rtw, name, mode="sah", tuning=None):
    cam, _ = S.cameras(*S.SHAPES[name])
    return S.render(rtw, S.arrays(rtw, name, mode), cam, device=0, tuning=tuning)


@pytest.mark.parametrize("mode", ["sah", "reference"])
def test_cluster_vs_oracle(rtw, mode):
    got = gpu_image(rtw, "cluster", mode)
    ref = S.oracle_image("cluster")
    assert np.isfinite(got).all() and (got[:, 3] == S.SPP).all()
    ok = S.close(got[:, :3], ref[:, :3], REL)
    assert ok.all(), (ok.mean(), np.abs(got[:, :3] - ref[:, :3]).max())


TUNINGS = [{"kernel": 1}, {"kernel": 2}, {"fuse": 0}, {"fuse": 3}, {"fuse": 7}, {"lds": 127 & ~16},
           {"deal": 0}, {"deal": 59, "sort_iters": 50, "sort_iters_split": 50},
           {"deal": 187, "sort_iters": 50, "sort_iters_split": 50}, {"deal": 0, "sort_iters": 50, "sort_iters_split": 50},
           {"fast_box": 0}, {"fast_box": 0, "kernel": 1}, {"fuse": 0, "lds": 127 & ~16}]


@pytest.mark.parametrize("name", ["cluster", "medium"])
def test_gpu_equals_host_and_every_kernel(rtw, name):
    """One image: the host backend's, the default wavefront's, the persistent and simple kernels', fused or
    split steps, geometry staged in LDS or not, every dealing mode with bucketed queues, both slab tests."""
    host = S.host_image(name)
    assert np.array_equal(gpu_image(rtw, name), host)
    for tu in TUNINGS:
        assert np.array_equal(gpu_image(rtw, name, tuning=tu), host), tu


@pytest.mark.parametrize("pair", [("cornell_tree", "cornell_list"), ("rot12_tree", "rot12_list"),
                                  ("cluster", "cluster3")])
def test_tree_equals_list(rtw, pair):
    a, b = gpu_image(rtw, pair[0]), gpu_image(rtw, pair[1])
    assert np.array_equal(a, b)
    assert np.array_equal(a, S.host_image(pair[0]))


def test_reduced_final_scene(rtw):
    ref = S.oracle_image("final")
    got = gpu_image(rtw, "final", "reference")
    assert np.isfinite(got).all() and (got[:, 3] == S.SPP).all()
    ok = S.close(got[:, :3], ref[:, :3], REL)
    assert ok.all(), (ok.mean(), np.abs(got[:, :3] - ref[:, :3]).max())
    assert np.array_equal(gpu_image(rtw, "final", "sah"), S.host_image("final", "sah"))

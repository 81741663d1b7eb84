"""Every kernel variant the launcher can pick, against the oracle, with proof of which kernel ran.

One case per row of tests/kernel_variant_cases.py (tests/test_kernel_resources_cpu.py holds that table to the compiled library: no
instantiation without a row).  A row renders through pt_render, compares with the oracle bit for bit, and reads the kernels of both
passes back through pt_debug_last_kernels: the frame pass must be the row's kernel, the cost-probe pass the parity-mode kernel the row
states.  The launcher probes frames of 64 tiles and more, so a row renders twice: 61 x 35 x 20 (40 tiles, padding pixels on both edges:
the frame pass alone, and no probe tag) and 61 x 67 x 16 (72 tiles: the kernel as the cost probe and as the frame pass that resumes its
samples).  Fast-mode rows: 70 and 66 samples against the oracle's fast mode (one chunk and a partial one)."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import kernel_variant_cases as K
from conftest import assert_bit_identical
from path_tracer_amd import abi, scenes
from path_tracer_amd import render as R
from test_aov_cpu import PLANES, aov_np
from test_gpu_aov import host, last_aov, same_planes
from test_gpu_fuzz import tri_pools

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


def device_scene(lib, r, ps):
    """The row's DeviceScene, and the fact its kernel's extra code exists for: a kernel that runs with nothing to cull proves little."""
    with (tri_pools(**r.env) if r.env is not None else contextlib.nullcontext()):
        st = (C.c_int32 * 8)()
        abi.check(lib.pt_debug_tri_pool(C.byref(ps.desc), st), "pt_debug_tri_pool")
        ds = R.DeviceScene(ps, abi.tuning(**r.tuning) if r.tuning is not None else None)
    if r.fact == "grid":
        assert st[7] > 0, "the scene must have spheres in a culling grid"
    if r.fact == "tri_pool":
        assert st[0] > 0, "the scene's triangle run must get a pool"
    return ds


@pytest.mark.parametrize("r", K.ROWS, ids=K.row_id)
def test_variant_is_exact_and_is_the_kernel_that_ran(torch, orc, lib, r):
    ps, cam = K.build(r)
    ds = device_scene(lib, r, ps)
    assert K.last_kernels(ds) == (None, None)
    orc.set_math(True)
    fast = r.flags & abi.PT_FLAG_FAST_RNG
    if r.flags & abi.PT_FLAG_SINGLE_STREAM:
        frames = [(20, 12, 4, False)]
    else:
        frames = [(61, 35, 70 if fast else 20, False), (61, 67, 66 if fast else 16, True)]
    for w, h, spp, probed in frames:
        c = scenes.make_camera(cam, w, h)
        fb = R.render(w, h, spp, ds, c, flags=r.flags)
        torch.cuda.synchronize()
        ref = orc.render(ps, c.c, w, h, spp, flags=r.flags & (abi.PT_FLAG_FAST_RNG | abi.PT_FLAG_SINGLE_STREAM))
        probe, frame = K.last_kernels(ds)
        print(f"{K.row_id(r)} {w}x{h}x{spp}: probe {probe} frame {frame}")
        assert_bit_identical(fb.cpu().numpy(), ref, f"{K.row_id(r)} {w}x{h}x{spp}")
        assert frame == r.tag, f"{w}x{h}: the frame pass ran {frame}, the row says {r.tag}"
        assert probe == (r.probe if probed else None), f"{w}x{h}: the probe pass ran {probe}, the row says {r.probe if probed else None}"


@pytest.mark.parametrize("r", K.AOV_ROWS, ids=K.row_id)
def test_aov_variant_is_exact_and_is_the_kernel_that_ran(torch, orc, lib, r):
    """All six planes against aov_np (tests/test_aov_cpu.py) at 19 x 13 x 6, and pt_debug_last_aov names the row's kernel."""
    ps, cam = K.build(r)
    ds = device_scene(lib, r, ps)
    w, h, n = 19, 13, 6
    c = scenes.make_camera(cam, w, h)
    got = host(R.render_aov(w, h, n, ds, c))
    _, img, walk = r.tag
    assert last_aov(ds) == (walk, img)
    same_planes(got, aov_np(orc, ps, c.c, w, h, n), K.row_id(r), PLANES)
    assert (got["id"] >= 0).any()

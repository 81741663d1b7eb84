"""Scenes that sit exactly on a size threshold, and their neighbours one step above, against the oracle bit for bit at depth 50
(tests/threshold_scenes.py holds the recipes, tests/test_threshold_scenes_cpu.py their sizes and the visibility of their last records).
Every case renders through pt_render, reads the frame pass's kernel back (pt_debug_last_kernels) — it must be the one the recipe
names: the side of the threshold the launcher really took — and prints the probed size, the range the recipe needs and the tag that ran.
An image of exactly 64 KB must be accepted (not PT_ERR_TOO_LARGE): its render is the assertion.  No tolerances.  The headline rect / box
scenes at the cold-state and the materials limits also run one Accumulator split (3 + 1 samples) and one masked adaptive window: the
resume path and the lanes outside the mask read the same cold records and the same staged image.  Every reference is computed once per
scene, size and sample count and shared, read-only."""
import numpy as np
import pytest

import kernel_variant_cases as K
import threshold_scenes as T
from conftest import assert_bit_identical
from path_tracer_amd import abi, scenes
from path_tracer_amd import render as R

pytestmark = pytest.mark.gpu

_SCENES, _REFS = {}, {}


def _scene(r):
    """the recipe's scene, built once (rows that differ in flags or launch knobs alone share it)"""
    ps, cam = r.make()
    key = (bytes(ps.hittables), bytes(ps.materials), bytes(ps.textures), ps.n_hittables, ps.n_materials)
    return _SCENES.setdefault(key, (ps, cam, len(_SCENES)))


def _reference(orc, r, w, h, spp):
    ps, cam, index = _scene(r)
    fast = r.flags & abi.PT_FLAG_FAST_RNG
    key = (index, w, h, spp, fast)
    if key not in _REFS:
        orc.set_math(True)
        ref = orc.render(ps, scenes.make_camera(cam, w, h).c, w, h, spp, 50, flags=fast)
        ref.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def _tuning(r):
    return abi.tuning(**r.tuning) if r.tuning else abi.tuning()  # (explicit, as the probes were given it: the environment is not consulted)


def _ran(r, tag):
    name, members = r.tag
    return K.ran(tag, name, **members)


@pytest.mark.parametrize("name", [r.name for r in T.RECIPES])
def test_threshold_scene_is_exact_on_the_kernel_its_side_names(orc, name):
    r = T.by_name(name)
    ps, cam, _ = _scene(r)
    size = r.size(ps, r.tuning)
    assert r.expect[0] <= size <= r.expect[1], (name, size, r.expect)
    ds = R.DeviceScene(ps, _tuning(r))
    try:
        for w, h in r.frames:
            fb = R.render_host(w, h, r.spp, ds, scenes.make_camera(cam, w, h), 50, flags=r.flags)  # (accepted: a refusal raises)
            tag = K.last_kernels(ds)[1]
            print(f"{name} {w}x{h}x{r.spp}: {ps.n_hittables} hittables, probed {size}, needs {r.expect}, ran {tag}")
            assert _ran(r, tag), f"{name} {w}x{h}: the frame pass ran {tag}, the recipe says {r.tag}"
            assert_bit_identical(fb, _reference(orc, r, w, h, r.spp), f"{name} {w}x{h}x{r.spp}")
    finally:
        ds.close()


@pytest.mark.parametrize("name", ["T1-a-at", "T2-a-at"])
def test_split_and_masked_windows_on_the_limit(orc, name):
    """3 + 1 samples through an Accumulator equal one render of 4; an adaptive accumulator's masked fourth sample leaves every pixel at
    the bits of its own count"""
    import torch

    r = T.by_name(name)
    ps, cam, _ = _scene(r)
    ds = R.DeviceScene(ps, _tuning(r))
    try:
        for w, h in r.frames:
            c = scenes.make_camera(cam, w, h)
            ref3, ref4 = _reference(orc, r, w, h, 3), _reference(orc, r, w, h, 4)
            acc = R.Accumulator(w, h, ds, c)
            try:
                for window in (3, 1):
                    acc.add(window)
                    torch.cuda.synchronize()
                    assert _ran(r, K.last_kernels(ds)[1]), (name, window, K.last_kernels(ds))
                assert_bit_identical(acc.resolve().cpu().numpy(), ref4, f"{name} {w}x{h}: windows of 3 + 1 samples")
            finally:
                acc.close()
            mask = np.zeros((h, w), np.uint8)
            mask[h // 4:h - h // 4, w // 3:] = 1  # the marker's pixels and the right edge, padding lanes beside it
            mask[::3, ::5] ^= 1
            acc = R.Accumulator(w, h, ds, c, adaptive=True)
            try:
                acc.add(3)
                acc.add(1, torch.from_numpy(mask).cuda())
                torch.cuda.synchronize()
                tag = K.last_kernels(ds)[1]
                print(f"{name} {w}x{h}: masked window of {int(mask.sum())} pixels ran {tag}")
                assert _ran(r, tag), (name, tag)
                got = acc.resolve().cpu().numpy()
                assert (acc.counts().cpu().numpy() == 3 + mask).all()
            finally:
                acc.close()
            assert_bit_identical(got, np.where(mask[:, :, None] != 0, ref4, ref3), f"{name} {w}x{h}: 3 samples + 1 under a mask")
    finally:
        ds.close()

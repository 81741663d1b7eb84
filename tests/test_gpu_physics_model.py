"""The device against the independent binary64 model (tests/physics_model.py) directly, not through the oracle: the same
cases and the same compare() as tests/test_physics_model_cpu.py, with the records taken from the two existing probes,
pt_debug_bounce and pt_debug_camera_rays.  A failure here names the device even if the bit-exact tests were red."""
import ctypes as C

import pytest

import physics_cases as PC
from path_tracer_amd import abi
from path_tracer_amd import render as R
from physics_compare import compare
from test_gpu_fuzz import forced_pools

pytestmark = pytest.mark.gpu


def device_bounce(lib, case):
    n = len(case.recs)
    out = (abi.PtBounceOut * n)()
    ds = R.DeviceScene(case.ps)
    abi.check(lib.pt_debug_bounce(ds.handle, case.recs, out, n), "pt_debug_bounce")
    return out


def device_camera_rays(lib, case):
    n = len(case.states)
    out = (abi.PtCameraRay * n)()
    abi.check(lib.pt_debug_camera_rays(C.byref(case.cam), case.width, case.height, case.xy.ctypes.data_as(C.POINTER(C.c_int32)),
                                       case.states.ctypes.data_as(C.POINTER(C.c_uint32)), out, n), "pt_debug_camera_rays")
    return out


@pytest.mark.parametrize("name", PC.BOUNCE_NAMES)
def test_device_bounce_agrees_with_the_model(lib, name):
    case = PC.bounce_case(name)
    compare(device_bounce(lib, case), case, f"device {name}")


@pytest.mark.parametrize("name", PC.POOLED)
def test_device_bounce_agrees_with_the_model_with_forced_pools(lib, name):
    case = PC.bounce_case(name)
    with forced_pools():
        out = device_bounce(lib, case)
    compare(out, case, f"device {name}, pools forced")


@pytest.mark.parametrize("name", PC.CAMERA_NAMES)
def test_device_camera_rays_agree_with_the_model(lib, name):
    case = PC.camera_case(name)
    compare(device_camera_rays(lib, case), case, f"device camera {name}")

"""The CPU oracle against an independent binary64 model of one bounce and of the camera (tests/physics_model.py), over the
cases of tests/physics_cases.py, through tests/physics_compare.py::compare; and the proof that the comparison has teeth:
single-line wrong versions of oracle/pt_oracle.c, compiled beside the real one, must each fail it."""
import json
import math
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest

import physics_cases as PC
import physics_model as M
from path_tracer_amd import abi
from physics_compare import compare, compare_camera_fields

ROOT = Path(__file__).resolve().parent.parent
ORACLE_DIR = ROOT / "oracle"
GOLDEN = Path(__file__).resolve().parent / "golden"


def run_bounce_case(o, name, portable):
    case = PC.bounce_case(name)
    o.set_math(portable)
    return compare(o.bounce(case.ps, case.recs), case, f"{name} ({'portable' if portable else 'libm'} math)")


def run_camera_case(o, name, portable):
    case = PC.camera_case(name)
    o.set_math(portable)
    a = case.ctor_args
    a3 = lambda v: [float(np.float32(x)) for x in v]  # noqa: E731
    cam = o.camera_init(a3(a[0]), a3(a[1]), a3(a[2]), *a[3:])
    fields = compare_camera_fields(cam, a, f"camera {name}: constructor")
    stats = compare(o.camera_rays(cam, case.width, case.height, case.xy, case.states), case, f"camera {name}: get_ray")
    return fields, stats


@pytest.mark.parametrize("portable", [True, False], ids=["portable", "libm"])
@pytest.mark.parametrize("name", PC.BOUNCE_NAMES)
def test_oracle_bounce_agrees_with_the_model(orc, name, portable):
    try:
        run_bounce_case(orc, name, portable)
    finally:
        orc.set_math(False)


@pytest.mark.parametrize("portable", [True, False], ids=["portable", "libm"])
@pytest.mark.parametrize("name", PC.CAMERA_NAMES)
def test_oracle_camera_agrees_with_the_model(orc, name, portable):
    try:
        run_camera_case(orc, name, portable)
        # the product's host constructor (pt_camera_init) builds the camera the rays were drawn from: hold it too
        case = PC.camera_case(name)
        compare_camera_fields(case.cam, case.ctor_args, f"camera {name}: the product's constructor")
    finally:
        orc.set_math(False)


def test_model_xorshift_matches_the_reference_known_answers():
    kat = json.loads((GOLDEN / "xorshift32_kat.json").read_text())
    assert kat["streams"]
    for seed, stream in kat["streams"].items():
        x = int(seed)
        for want in stream:
            x = M.xorshift32(x)
            assert x == want, f"seed {seed}"
    for y in (1, 2463534242, 0xFFFFFFFF, 2 ** 31):
        assert M.xorshift32(M.xorshift32_inverse(y)) == y


def test_sampler_identities(orc):
    """Independent of how the samplers are restated: a Lambertian direction minus the normal has length 1; a metal's
    direction minus the mirror direction, over the fuzz, and an isotropic direction lie in the unit ball.  The slack is the
    rounding of the recorded binary32 components (sum and square root of three: 8 U relative) and, for the metal, of the
    difference of two O(1) vectors divided by the fuzz."""
    U = M.U
    for portable in (True, False):
        orc.set_math(portable)
        for name, kind in (("sphere_lambertian_solid", "lambertian"), ("yz_rect_lambertian_checker", "lambertian"),
                           ("sphere_moving_metal", "metal"), ("triangle_metal", "metal"), ("medium_sphere_isotropic", "isotropic")):
            case = PC.bounce_case(name)
            out = orc.bounce(case.ps, case.recs)
            seen = 0
            for k, (val, bnd, T) in enumerate(case.rows()):
                o = out[k]
                if o.status == abi.PT_BOUNCE_MISS or (kind != "metal" and o.status != abi.PT_BOUNCE_SCATTERED):
                    continue
                sd, n = np.array(o.sc_dir, dtype=np.float64), np.array(o.normal, dtype=np.float64)
                if kind == "lambertian":
                    assert abs(np.linalg.norm(sd - n) - 1.0) <= 16 * U, (name, k)
                elif kind == "isotropic":
                    assert np.linalg.norm(sd) <= 1.0 + 16 * U, (name, k)
                else:
                    if o.status != abi.PT_BOUNCE_SCATTERED:
                        continue   # an absorbed metal ray records no direction
                    d = np.array(case.recs[k].dir, dtype=np.float64)
                    ud = d / np.linalg.norm(d)
                    refl = ud - 2 * np.dot(ud, n) * n
                    fuzz = case.scene.m[o.material][3]
                    slack = (sum(bnd["sc_dir"]) + 16 * U) / fuzz
                    assert np.linalg.norm((sd - refl) / fuzz) <= 1.0 + slack, (name, k)
                seen += 1
            assert seen >= 30, name
    orc.set_math(False)


def test_unit_vec_half_states_draw_exactly_half():
    for st in PC.unit_vec_half_states()[:3]:
        r = M.Rng(st)
        r.float_t(), r.float_t()
        assert r.float_t() == 0.5
    for st in PC.unit_vec_half_states()[6:]:
        r = M.Rng(st)
        r.float_t(), r.float_t()
        assert r.float_t() != 0.5


# ---- the model rejects wrong oracles -------------------------------------------------------------------------------------

ALL_BOUNCE = tuple(PC.BOUNCE_NAMES)
# name: (old text, new text, what to run: bounce case names or "camera"); the old text must occur exactly once
MUTANTS = {
    "far sphere root tried first": ("float temp = (-b - sqrtf(discriminant)) / a;", "float temp = (-b + sqrtf(discriminant)) / a;",
                                    ("sphere_lambertian_solid", "edge_sphere")),
    "outward normal divided by |radius|": ("float radius = f[6];", "float radius = fabsf(f[6]);", ("sphere_hollow_dielectric", "edge_sphere_hollow")),
    "tmin 0.01": ("case PT_HIT_SPHERE: hit = sphere_hit(c, h->f, r, 0.001f,", "case PT_HIT_SPHERE: hit = sphere_hit(c, h->f, r, 0.01f,",
                  ("edge_sphere", "sphere_lambertian_solid", "sphere_dielectric")),
    "closest_so_far never narrowed": ("      *material = h->material;", "      *material = h->material; closest_so_far = PT_INF;",
                                      ("list_mixed", "list_cornell")),
    "moving centre without - time0": ("(time - time0) / (time1 - time0)", "(time) / (time1 - time0)", ("sphere_moving_metal", "edge_sphere_moving")),
    "xz_rect's in-plane axes swapped": ("oa = r->orig.x; da = r->dir.x; ob = r->orig.z; db = r->dir.z; n = V(0, 1, 0);",
                                        "oa = r->orig.z; da = r->dir.z; ob = r->orig.x; db = r->dir.x; n = V(0, 1, 0);", ("xz_rect_light", "edge_xz_rect")),
    "rectangle v from the a range": ("rec->v = (b - b0) / (b1 - b0);", "rec->v = (b - b0) / (a1 - a0);", ("xy_rect_lambertian_image", "yz_rect_image")),
    "triangle normal cross(edge2, edge1)": ("set_face_normal(rec, r, vcross(edge1, edge2));", "set_face_normal(rec, r, vcross(edge2, edge1));",
                                            ("triangle_lambertian", "triangle_dielectric")),
    "a box side at the wrong bound": ("rect_hit(c, 0, x0, x1, y0, y1, z1, r", "rect_hit(c, 0, x0, x1, y0, y1, z0, r", ("box_metal", "edge_box")),
    "medium t without / ray_length": ("rec->t = rec1.t + hit_distance / ray_length;", "rec->t = rec1.t + hit_distance;",
                                      ("medium_sphere_isotropic", "medium_box_isotropic_checker")),
    "medium exit searched from entry - offset": ("rec1.t + 0.0001f", "rec1.t - 0.0001f", ("medium_sphere_isotropic", "medium_box_isotropic_checker")),
    "reflect with factor 1": ("vscale(2.0f * vdot(v, n), n)", "vscale(1.0f * vdot(v, n), n)", ("box_metal", "sphere_dielectric")),
    "refraction ratio inverted": ("rec->front_face ? (1.0f / ref_idx) : ref_idx", "rec->front_face ? ref_idx : (1.0f / ref_idx)",
                                  ("sphere_dielectric", "xz_rect_dielectric")),
    "Schlick on cosine": ("m_pow5(1.0f - cosine)", "m_pow5(cosine)", ("sphere_dielectric", "edge_dielectric_angles")),
    "metal absorbing on < 0": ("return vdot(scattered->dir, rec->normal) > 0;", "return vdot(scattered->dir, rec->normal) < 0;",
                               ("sphere_moving_metal", "box_metal")),
    "Mercator u without the 1 -": ("*u = 1.0f - (phi + PT_PI) / (2.0f * PT_PI);", "*u = (phi + PT_PI) / (2.0f * PT_PI);", ("sphere_lambertian_image",)),
    "image v without the flip": ("(1.0f - m_fmod1(rec->v * t->freq)) * (float)(t->height - 1)", "(m_fmod1(rec->v * t->freq)) * (float)(t->height - 1)",
                                 ("sphere_lambertian_image", "xy_rect_lambertian_image")),
    "checker sign reversed": ("if (sines < 0) return vld(t->color0);", "if (sines > 0) return vld(t->color0);", ("yz_rect_lambertian_checker", "sphere_checker")),
    "emission multiplied by the attenuation": ("vst(o->color, emitted);", "vst(o->color, vmul(att, emitted));", ("xz_rect_light", "sphere_light")),
    "camera vertical from the viewport width": ("vscale(focus_dist * viewport_height, v)", "vscale(focus_dist * viewport_width, v)", "camera"),
    "get_ray direction without - offset": ("origin), offset);", "origin), V(0.0f, 0.0f, 0.0f));", "camera"),
    "unit_vec choosing z on >= 0.5": ("(rng_float(c) > 0.5f) ? absz : -absz", "(rng_float(c) >= 0.5f) ? absz : -absz", ("edge_sphere",)),
}


def makefile_cflags():
    text = (ORACLE_DIR / "Makefile").read_text()
    flags = re.search(r"^CFLAGS\s*=\s*(.*)$", text, re.M).group(1).split()
    assert "-O3" in flags and "-ffp-contract=off" in flags
    return ["-O1" if f == "-O3" else f for f in flags]


def compile_oracle(text, out_dir: Path, stem: str):
    src = out_dir / f"{stem}.c"
    src.write_text(text)
    so = out_dir / f"lib{stem}.so"
    subprocess.run(["gcc", *makefile_cflags(), f"-I{ORACLE_DIR}", "-shared", "-o", str(so), str(src), "-lm"], check=True, cwd=str(out_dir))
    return so


@pytest.fixture(scope="module")
def mutant_libraries(tmp_path_factory):
    """name -> path of the shared library; "" is the unchanged text compiled the same way."""
    out_dir = tmp_path_factory.mktemp("oracle_mutants")
    text = (ORACLE_DIR / "pt_oracle.c").read_text()
    jobs = {"": text}
    for name, (old, new, _) in MUTANTS.items():
        assert text.count(old) == 1, f"mutant '{name}': its old text occurs {text.count(old)} times in pt_oracle.c"
        jobs[name] = text.replace(old, new)
    with ThreadPoolExecutor(max_workers=16) as pool:
        futures = {name: pool.submit(compile_oracle, t, out_dir, f"m{k}") for k, (name, t) in enumerate(jobs.items())}
        return {name: f.result() for name, f in futures.items()}


def test_unchanged_oracle_compiled_like_the_mutants_passes_everything(mutant_libraries):
    from oracle import binding
    o = binding.bind(mutant_libraries[""])
    for portable in (True, False):
        for name in PC.BOUNCE_NAMES:
            run_bounce_case(o, name, portable)
        for name in PC.CAMERA_NAMES:
            run_camera_case(o, name, portable)


KILLS = {}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_model_rejects_a_wrong_oracle(mutant_libraries, mutant):
    from oracle import binding
    o = binding.bind(mutant_libraries[mutant])
    targets = MUTANTS[mutant][2]
    killed = []
    for name in (PC.CAMERA_NAMES if targets == "camera" else targets):
        try:
            if targets == "camera":
                run_camera_case(o, name, True)
            else:
                run_bounce_case(o, name, True)
        except AssertionError as e:
            killed.append((name, str(e).splitlines()[0]))
    KILLS[mutant] = killed
    assert killed, f"the comparison lets the mutant '{mutant}' through on {targets}"
    if mutant == "unit_vec choosing z on >= 0.5":
        # it must be caught by a decided ray whose third draw is exactly 0.5, through sc_dir
        case = PC.bounce_case("edge_sphere")
        out = o.bounce(case.ps, case.recs)
        halves = set(PC.unit_vec_half_states()[:3])
        hit = [k for k, (val, bnd, T) in enumerate(case.rows()) if int(case.recs[k].rng_state) in halves and not T.borderline()
               and val["status"] == abi.PT_BOUNCE_SCATTERED and not math.isclose(out[k].sc_dir[2], val["sc_dir"][2], abs_tol=1e-3)]
        assert hit, "no decided ray with a sign draw of exactly 0.5 shows the mutant"

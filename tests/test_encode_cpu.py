"""CPU tests of the encode stage's boundary and definition (include/pt_encode.h: pt_encode, pt_display_encode).  The two tables of the
header are verified entry by entry with integer arithmetic alone — fractions.Fraction decides x >= EOTF(v) exactly, no libm and no
tolerance.  The new header is held to the rules include/pt_render.h is held to by tests/test_abi_cpu.py and
tests/test_stream_contract_cpu.py, as tests/test_metrics_cpu.py holds pt_metrics.h: abi.ENCODE_SIGNATURES is exactly what it declares, the
library exports all of it, and every prototype with a `void* stream` has a row in the contract table below and a comment that says what
the row says.  The struct and the defaults are the header's; every refusal is pinned alone and, with doubly wrong calls, in each entry
point's own order, on the host with made-up addresses; the restatement of the header (tests/encode_model.py, the one
tests/test_gpu_encode.py holds the kernel to) is held to the properties of the definition; the PNG writers tag what they are told to and
nothing else, the CLI options parse and are refused without a GPU, and the facade's program compiles."""
import ctypes as C
import hashlib
import math
import re
import struct
import subprocess
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import encode_model as E
from path_tracer_amd import abi

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "pt_encode.h"
OTHER_HEADERS = [ROOT / "include" / n for n in ("pt_render.h", "pt_post.h", "pt_spatial_variance.h", "pt_metrics.h")]
F = np.float32

# The stream contract of include/pt_encode.h, one row per prototype with a `void* stream` parameter: "async" — the call is asynchronous on
# `stream` —, or "sync" — it synchronises `stream`.
ENCODE_CONTRACT = {
    "pt_encode": "async",
    "pt_display_encode": "async",
}
ASYNC = re.compile(r"asynchronous on `stream`", re.I)
SYNC = re.compile(r"\bsynchronis\w* `stream`", re.I)
PROTO = re.compile(r"^(?:extern\s+)?(int|void|int32_t|int64_t|uint32_t|const char\*)\s+(pt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", re.M)


def header_code(path=HEADER):
    """The header with its comments blanked in place (offsets stay the file's)."""
    return re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), path.read_text(), flags=re.S)


def prototypes(path=HEADER):
    """{name: (return type, [parameter declarations], offset)}"""
    return {m.group(2): (m.group(1), [re.sub(r"\s+", " ", a.strip()) for a in m.group(3).split(",")], m.start())
            for m in PROTO.finditer(header_code(path))}


# ---- the tables: exact, by integers -----------------------------------------------------------------------------------------------------

def at_least_eotf(x: Fraction, v: Fraction) -> bool:
    """x >= EOTF(v) for IEC 61966-2-1's decoding function, decided exactly: 2.4 = 12/5, so the power branch is x^5 >= (...)^12."""
    if v <= Fraction(4045, 100000):
        return x >= v / Fraction(1292, 100)
    return x ** 5 >= ((v + Fraction(55, 1000)) / Fraction(1055, 1000)) ** 12


def bits_of(x) -> int:
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def float_of(b: int) -> float:
    return struct.unpack("<f", struct.pack("<I", b))[0]


def test_the_macros_hold_255_and_256_binary32_hex_floats():
    text = HEADER.read_text()
    for name, n in (("PT_SRGB8_THRESHOLDS", 255), ("PT_SRGB8_LEVELS", 256)):
        body = re.search(r"#define %s \{(.*?)\}" % name, text, re.S).group(1).replace("\\\n", " ")
        items = [v.strip() for v in body.split(",")]
        assert len(items) == n, name
        for v in items:
            assert re.fullmatch(r"0x[01](\.[0-9a-f]{6})?p[+-]\d+f", v), (name, v)  # at most 24 significant bits: a binary32, exactly
            assert float(F(float.fromhex(v[:-1]))) == float.fromhex(v[:-1]), (name, v)
    assert E.M.dtype == F and E.L.dtype == F and E.M.shape == (255,) and E.L.shape == (256,)


def test_every_threshold_is_the_smallest_binary32_at_or_above_the_exact_boundary():
    for c in range(1, 256):
        v = Fraction(2 * c - 1, 510)
        b = bits_of(E.M[c - 1])
        assert at_least_eotf(Fraction(float_of(b)), v), c
        assert not at_least_eotf(Fraction(float_of(b - 1)), v), c  # its binary32 predecessor is below the boundary


def test_every_level_is_the_smallest_binary32_at_or_above_the_exact_level():
    assert bits_of(E.L[0]) == 0  # +0
    for c in range(1, 256):
        v = Fraction(c, 255)
        b = bits_of(E.L[c])
        assert at_least_eotf(Fraction(float_of(b)), v), c
        assert not at_least_eotf(Fraction(float_of(b - 1)), v), c
    assert bits_of(E.L[255]) == 0x3F800000  # exactly 1.0f


def test_anchors_digests_and_order():
    h = lambda s: F(float.fromhex(s))
    assert E.M[0] == h("0x1.3e4568p-13") and E.M[9] == h("0x1.79f26cp-9") and E.M[10] == h("0x1.a1e5a2p-9")
    assert E.M[127] == h("0x1.b65b34p-3") and E.M[254] == h("0x1.fdb81cp-1") and E.L[1] == h("0x1.3e4568p-12")
    assert Fraction(2 * 10 - 1, 510) <= Fraction(4045, 100000) < Fraction(2 * 11 - 1, 510)  # M[10] is the last of the linear branch
    assert hashlib.sha256(E.M.astype("<f4").tobytes()).hexdigest().startswith("0b408a80ff623c35")
    assert hashlib.sha256(E.L.astype("<f4").tobytes()).hexdigest().startswith("28d477d3d14152f2")
    assert (np.diff(E.M.astype(np.float64)) > 0).all() and (np.diff(E.L.astype(np.float64)) > 0).all()
    for c in range(255):
        assert E.L[c] < E.M[c] < E.L[c + 1], c  # L[c] < M[c + 1] < L[c + 1]
    assert not np.isnan(E.M).any() and (E.M >= F(2.0 ** -126)).all() and (E.L[1:] >= F(2.0 ** -126)).all()  # no subnormal entry


def test_the_bayer_matrix_is_the_headers():
    u, v = np.meshgrid(np.arange(8), np.arange(8))
    b = E.bayer(u, v)  # [v][u]
    assert list(b[0]) == [0, 32, 8, 40, 2, 34, 10, 42]
    assert sorted(b.ravel()) == list(range(64))
    t = E.thresholds(8, 8)
    assert t.dtype == F and t.min() == F(0.5 / 64) and t.max() == F(63.5 / 64)
    assert (t.astype(np.float64) == (b + 0.5) / 64).all()  # exact
    assert (E.thresholds(8, 8, (-1, 9)) == np.roll(np.roll(t, 1, axis=1), -1, axis=0)).all()  # & 7 on the two's-complement sum
    assert "0 32 8 40 2 34 10 42" in HEADER.read_text()


# ---- the boundary -------------------------------------------------------------------------------------------------------------------

def ctype_of(decl):
    """The ctypes type abi.py gives a parameter declared as `decl`: pointers to device memory, states and streams are void pointers."""
    if re.fullmatch(r"(const )?PtEncodeParams\* \w+", decl):
        return C.POINTER(abi.PtEncodeParams)
    if re.fullmatch(r"(const )?PtDisplayParams\* \w+", decl):
        return C.POINTER(abi.PtDisplayParams)
    if re.fullmatch(r"int32_t \w+\[\d+\]", decl):
        return C.POINTER(C.c_int32)
    if re.fullmatch(r"(const )?(float|uint8_t|void|PtDisplay)\* \w+", decl):
        return C.c_void_p
    if re.fullmatch(r"int32_t \w+", decl):
        return C.c_int32
    raise AssertionError(f"no rule for the parameter {decl!r}")


def test_signatures_are_exactly_what_the_header_declares(lib):
    protos = prototypes()
    table = abi.ENCODE_SIGNATURES
    assert set(protos) == set(table) == set(abi.ENCODE_SYMBOLS), sorted(set(protos) ^ set(table))
    ret = {"int": C.c_int, "void": None, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "const char*": C.c_char_p}
    for name, (rtype, args, _) in protos.items():
        want_args = [] if args == ["void"] else [ctype_of(a) for a in args]
        assert table[name] == (ret[rtype], want_args), name
        assert hasattr(lib, name), f"libpt_render.so does not export {name}"
        fn = getattr(lib, name)
        assert fn.restype == table[name][0] and list(fn.argtypes) == table[name][1], name  # load_library applied the row
    assert abi.has_encode(lib)
    assert protos["pt_encode"][:2] == ("int", ["const PtEncodeParams* params", "const float* linear", "uint8_t* rgb8_out", "void* stream"])
    assert protos["pt_display_encode"][:2] == ("int", ["const PtDisplay* state", "const PtDisplayParams* display_params",
                                                       "const PtEncodeParams* encode_params", "const float* color", "uint8_t* rgb8_out",
                                                       "void* stream"])
    assert protos["pt_encode_params_init"][:2] == ("void", ["PtEncodeParams* params", "int32_t width", "int32_t height"])
    assert protos["pt_debug_last_encode"][:2] == ("int", ["int32_t out[8]"])


def test_the_tables_and_the_headers_are_disjoint(lib):
    others = (abi.SIGNATURES, abi.POST_SIGNATURES, abi.SPATIAL_VARIANCE_SIGNATURES, abi.METRICS_SIGNATURES)
    for table in others:
        assert not set(abi.ENCODE_SIGNATURES) & set(table)
    for other in OTHER_HEADERS:
        assert not set(prototypes()) & set(prototypes(other)), other
        assert "pt_encode" not in other.read_text() and "PT_SRGB8" not in other.read_text(), other  # the older headers know nothing of the stage
    assert '#include "pt_render.h"' in HEADER.read_text()  # the error codes, PtDisplay and pt_last_error are its
    assert lib.pt_abi_version() == 2                        # detected by the symbols, not by a version


def struct_fields(name):
    body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s;" % (name, name), header_code(), re.S).group(1)
    fields = []
    ctypes_of = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "float": C.c_float}
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = re.match(r"(int32_t|uint32_t|float)\s+(.*)", decl).groups()
            fields += [(nm.strip(), ctypes_of[ctype]) for nm in names.split(",")]
    return fields


def test_the_struct_matches_the_header():
    fields = struct_fields("PtEncodeParams")
    assert [n for n, _ in fields] == ["struct_size", "width", "height", "transfer", "flags", "phase_x", "phase_y", "reserved"]
    assert abi.PtEncodeParams._fields_ == fields
    assert C.sizeof(abi.PtEncodeParams) == 32


def test_defaults_are_the_headers(lib):
    text = HEADER.read_text()
    m = dict(re.findall(r"^#define (PT_(?:ENCODE|TRANSFER)_\w+) (\S+)", text, re.M))
    p = abi.PtEncodeParams()
    C.memset(C.byref(p), 7, C.sizeof(p))
    lib.pt_encode_params_init(C.byref(p), 64, 40)
    assert (p.struct_size, p.width, p.height, p.reserved) == (C.sizeof(abi.PtEncodeParams), 64, 40, 0)
    assert (p.transfer, p.flags, p.phase_x, p.phase_y) == (abi.PT_TRANSFER_SRGB, 0, 0, 0)  # sRGB, no dither, phase 0
    assert int(m["PT_TRANSFER_REFERENCE"]) == abi.PT_TRANSFER_REFERENCE == E.REFERENCE == 0
    assert int(m["PT_TRANSFER_SRGB"]) == abi.PT_TRANSFER_SRGB == E.SRGB == 1
    assert int(m["PT_ENCODE_DITHER"].rstrip("u")) == abi.PT_ENCODE_DITHER == E.DITHER == 1
    assert int(m["PT_ENCODE_NO_VEC"].rstrip("u")) == abi.PT_ENCODE_NO_VEC == E.NO_VEC == 2
    assert m["PT_ENCODE_DEFAULT_TRANSFER"] == "PT_TRANSFER_SRGB" and abi.PT_ENCODE_DEFAULT_TRANSFER == abi.PT_TRANSFER_SRGB
    assert int(m["PT_ENCODE_DEFAULT_FLAGS"].rstrip("u")) == abi.PT_ENCODE_DEFAULT_FLAGS == 0
    assert abi.TRANSFERS == {"reference": 0, "srgb": 1}
    lib.pt_encode_params_init(None, 1, 1)  # a NULL struct is ignored


def words(comment):
    return re.sub(r"\s+", " ", re.sub(r"^\s*\*", " ", comment, flags=re.M))


def test_every_prototype_with_a_stream_has_a_row_and_a_comment_that_says_so():
    """tests/test_stream_contract_cpu.py's rule, for this header: the comment directly above the prototype says what the table says."""
    text = HEADER.read_text()
    protos = prototypes()
    with_stream = {n for n, (_, args, _) in protos.items() if any(re.search(r"\bvoid\s*\*\s*stream\b", a) for a in args)}
    assert with_stream == set(ENCODE_CONTRACT) == {"pt_encode", "pt_display_encode"}
    for name, want in ENCODE_CONTRACT.items():
        at = protos[name][2]
        found = list(re.finditer(r"/\*(?:(?!\*/).)*\*/", text[:at], re.S))
        assert found and text[found[-1].end():at].strip() == "", name  # directly above: nothing stands between
        own = words(found[-1].group(0))
        assert (bool(ASYNC.search(own)), bool(SYNC.search(own))) == (want == "async", want == "sync"), (name, own)
        assert abi.ENCODE_SIGNATURES[name][1][-1] == C.c_void_p, name  # abi.py passes it a stream


# ---- refusals: on the host, made-up aligned addresses, no device ---------------------------------------------------------------------

W, H = 64, 40
VALUES = W * H * 3
STATE, LINEAR, RGB8 = 0x10000000, 0x20000000, 0x30000000
BAD, LARGE = abi.PT_ERR_INVALID_ARG, abi.PT_ERR_TOO_LARGE
BIG = dict(width=1 << 16, height=(1 << 14) + 1)  # one row more than 2^30 pixels
SRGB, REF, DITHER = abi.PT_TRANSFER_SRGB, abi.PT_TRANSFER_REFERENCE, abi.PT_ENCODE_DITHER
UNSET = object()


def encode_params(lib, **over):
    p = abi.PtEncodeParams()
    lib.pt_encode_params_init(C.byref(p), W, H)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def display_params(lib, **over):
    p = abi.PtDisplayParams()
    lib.pt_display_params_init(C.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def call_encode(lib, fields=None, params=UNSET, linear=LINEAR, rgb8=RGB8):
    p = encode_params(lib, **(fields or {})) if params is UNSET else params
    return lib.pt_encode(C.byref(p) if p is not None else None, linear, rgb8, None)


def call_fused(lib, fields=None, dfields=None, params=UNSET, dparams=UNSET, state=STATE, color=LINEAR, rgb8=RGB8):
    p = encode_params(lib, **(fields or {})) if params is UNSET else params
    d = display_params(lib, **(dfields or {})) if dparams is UNSET else dparams
    return lib.pt_display_encode(state, C.byref(d) if d is not None else None, C.byref(p) if p is not None else None, color, rgb8, None)


def refused(lib, rc, want_rc, who, message):
    text = lib.pt_last_error().decode()
    assert rc == want_rc, (rc, text)
    assert text.startswith(who + ": ") and message in text, text


ALONE = [
    (dict(struct_size=0), BAD, "PtEncodeParams.struct_size is not this library's"),
    (dict(struct_size=28), BAD, "PtEncodeParams.struct_size is not this library's"),
    (dict(struct_size=36), BAD, "PtEncodeParams.struct_size is not this library's"),
    (dict(width=0), BAD, "width and height must be > 0"),
    (dict(height=0), BAD, "width and height must be > 0"),
    (dict(width=-1), BAD, "width and height must be > 0"),
    (dict(height=-3), BAD, "width and height must be > 0"),
    (dict(BIG), LARGE, "more than 2^30 pixels"),
    (dict(width=1 << 16, height=1 << 15), LARGE, "more than 2^30 pixels"),
    (dict(transfer=2), BAD, "unknown transfer"),
    (dict(transfer=-1), BAD, "unknown transfer"),
    (dict(flags=4), BAD, "unknown flags"),
    (dict(flags=1 << 31), BAD, "unknown flags"),
    (dict(transfer=REF, flags=DITHER), BAD, "PT_ENCODE_DITHER needs PT_TRANSFER_SRGB"),
    (dict(transfer=REF, flags=DITHER | abi.PT_ENCODE_NO_VEC), BAD, "PT_ENCODE_DITHER needs PT_TRANSFER_SRGB"),
]


@pytest.mark.parametrize("fields,rc,message", ALONE, ids=lambda v: ",".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_each_entry_point_refuses_bad_encode_params_before_touching_a_device(lib, fields, rc, message):
    refused(lib, call_encode(lib, fields), rc, "pt_encode", message)
    refused(lib, call_fused(lib, fields), rc, "pt_display_encode", message)
    refused(lib, call_fused(lib, fields, state=None), rc, "pt_display_encode", message)


def test_refuses_null_arguments(lib):
    refused(lib, call_encode(lib, params=None), BAD, "pt_encode", "NULL params, linear or rgb8_out")
    refused(lib, call_encode(lib, linear=None), BAD, "pt_encode", "NULL params, linear or rgb8_out")
    refused(lib, call_encode(lib, rgb8=None), BAD, "pt_encode", "NULL params, linear or rgb8_out")
    refused(lib, call_fused(lib, params=None), BAD, "pt_display_encode", "NULL encode_params or rgb8_out")
    refused(lib, call_fused(lib, rgb8=None), BAD, "pt_display_encode", "NULL encode_params or rgb8_out")
    refused(lib, call_fused(lib, dparams=None), BAD, "pt_display_encode", "NULL params or color")
    refused(lib, call_fused(lib, color=None), BAD, "pt_display_encode", "NULL params or color")
    assert lib.pt_debug_last_encode(None) == BAD and b"pt_debug_last_encode" in lib.pt_last_error()
    last = (C.c_int32 * 8)(*[9] * 8)
    assert lib.pt_debug_last_encode(last) == abi.PT_OK and 9 not in list(last)


def test_refuses_an_output_that_overlaps_the_input(lib):
    for call in (call_encode, call_fused):
        who = "pt_encode" if call is call_encode else "pt_display_encode"
        for rgb8 in (LINEAR, LINEAR + 1, LINEAR + 4 * VALUES - 1, LINEAR - VALUES + 1):
            refused(lib, call(lib, rgb8=rgb8), BAD, who, "rgb8_out overlaps the input")
    # (a plane one byte clear of the input is taken: tests/test_gpu_encode.py, with live planes)


RECT_OUT = dict(rect_x0=0, rect_y0=0, rect_x1=W + 1, rect_y1=H)
DISPLAY_REFUSALS = [  # what pt_display_apply refuses about display_params, with its strings
    (dict(struct_size=0), "PtDisplayParams.struct_size is not this library's"),
    (dict(tone=3), "unknown tone"),
    (dict(tone=-1), "unknown tone"),
    (dict(flags=1), "unknown flags"),
    (dict(lo_permille=-1), "need 0 <= lo_permille < hi_permille <= 1000"),
    (dict(adapt_up=0.0), "an adaptation rate is outside (0, 1]"),
    (dict(ev_min=-33.0), "need -32 <= ev_min <= ev_max <= 32"),
    (dict(ev_bias=math.nan), "ev_bias is not finite"),
    (dict(white=0.0), "white: 1 / (white * white)"),
    (RECT_OUT, "the metering rectangle is empty or leaves the frame"),
]


@pytest.mark.parametrize("dfields,message", DISPLAY_REFUSALS, ids=[",".join(d) for d, _ in DISPLAY_REFUSALS])
def test_the_fused_call_refuses_what_pt_display_apply_refuses_with_its_words(lib, dfields, message):
    refused(lib, call_fused(lib, dfields=dfields), BAD, "pt_display_encode", message)
    d = display_params(lib, **dfields)
    assert lib.pt_display_apply(STATE, C.byref(d), LINEAR, W, H, RGB8, None, None) == BAD
    assert lib.pt_last_error().decode().startswith("pt_display_apply: ") and message in lib.pt_last_error().decode()
    refused(lib, call_fused(lib, dict(width=1 << 16, height=(1 << 15) + 1)), BAD, "pt_display_encode", "more than 2^31 pixels")


# (entry point, encode fields, display fields, pointers, rc, message): every call is wrong in TWO ways; the first defect of the entry
# point's own order — the header's — is the one reported
OVERLAP = dict(rgb8=LINEAR + 8)
ORDER = [
    ("pt_encode", dict(struct_size=0, width=0), {}, dict(linear=None), BAD, "NULL params, linear or rgb8_out"),
    ("pt_encode", dict(struct_size=0, width=0), {}, {}, BAD, "struct_size is not this library's"),
    ("pt_encode", dict(width=0, transfer=5), {}, {}, BAD, "width and height must be > 0"),
    ("pt_encode", dict(transfer=5, **BIG), {}, {}, LARGE, "more than 2^30 pixels"),
    ("pt_encode", dict(transfer=5, flags=8), {}, {}, BAD, "unknown transfer"),
    ("pt_encode", dict(transfer=REF, flags=8 | DITHER), {}, {}, BAD, "unknown flags"),
    ("pt_encode", dict(transfer=REF, flags=DITHER), {}, OVERLAP, BAD, "PT_ENCODE_DITHER needs PT_TRANSFER_SRGB"),
    ("pt_encode", dict(flags=8), {}, OVERLAP, BAD, "unknown flags"),
    ("pt_display_encode", dict(struct_size=0), dict(struct_size=0), dict(rgb8=None), BAD, "NULL encode_params or rgb8_out"),
    ("pt_display_encode", dict(struct_size=0), {}, dict(color=None), BAD, "PtEncodeParams.struct_size is not this library's"),
    ("pt_display_encode", dict(struct_size=0), dict(struct_size=0), {}, BAD, "PtEncodeParams.struct_size is not this library's"),
    ("pt_display_encode", dict(width=0), dict(struct_size=0), dict(color=None), BAD, "NULL params or color"),
    ("pt_display_encode", dict(width=0), dict(struct_size=0), {}, BAD, "PtDisplayParams.struct_size is not this library's"),
    ("pt_display_encode", dict(width=0), dict(tone=3), {}, BAD, "width and height must be > 0"),
    ("pt_display_encode", dict(BIG), dict(tone=3), {}, BAD, "unknown tone"),
    ("pt_display_encode", dict(BIG), dict(rect_x0=0, rect_y0=0, rect_x1=(1 << 16) + 1, rect_y1=1), {}, BAD, "the metering rectangle is empty or leaves the frame"),
    ("pt_display_encode", dict(transfer=5, **BIG), {}, {}, LARGE, "more than 2^30 pixels"),
    ("pt_display_encode", dict(transfer=5, flags=8), {}, {}, BAD, "unknown transfer"),
    ("pt_display_encode", dict(transfer=REF, flags=8 | DITHER), {}, {}, BAD, "unknown flags"),
    ("pt_display_encode", dict(transfer=REF, flags=DITHER), {}, OVERLAP, BAD, "PT_ENCODE_DITHER needs PT_TRANSFER_SRGB"),
    ("pt_display_encode", dict(flags=8), {}, dict(rgb8=LINEAR + 8, state=None), BAD, "unknown flags"),
]


@pytest.mark.parametrize("entry,fields,dfields,ptrs,rc,message", ORDER, ids=[f"{e}-{i}" for i, (e, *_) in enumerate(ORDER)])
def test_the_first_defect_in_the_entry_points_own_order_is_the_one_reported(lib, entry, fields, dfields, ptrs, rc, message):
    if entry == "pt_encode":
        got = call_encode(lib, fields, **ptrs)
    else:
        got = call_fused(lib, fields, dfields, **ptrs)
    refused(lib, got, rc, entry, message)


def test_the_header_states_each_calls_order():
    text = words(HEADER.read_text())
    at = [text.index(s) for s in ("a NULL params, linear or rgb8_out", "a struct_size other than sizeof(PtEncodeParams)", "width or height <= 0",
                                  "more than 2^30 pixels (PT_ERR_TOO_LARGE)", "an unknown transfer", "flags other than PT_ENCODE_DITHER",
                                  "PT_ENCODE_DITHER with PT_TRANSFER_REFERENCE", "rgb8_out overlapping linear")]
    assert at == sorted(at)
    assert "each call in this order" in text


# ---- the model: properties of the definition --------------------------------------------------------------------------------------------

def flat(x, n=8):
    return np.full((n, n, 3), x, dtype=F)


def test_every_level_encodes_to_its_code_in_both_modes():
    frame = np.zeros((8, 32, 3), dtype=F)
    frame.reshape(-1)[:256] = E.L
    frame.reshape(-1)[256:512] = E.L
    frame.reshape(-1)[512:768] = E.L
    want = np.concatenate([np.arange(256)] * 3).astype(np.uint8)
    for dither in (False, True):
        for phase in ((0, 0), (3, 5)):
            got = E.encode(frame, E.SRGB, dither, phase)[::-1].reshape(-1)
            assert (got == want).all(), (dither, phase)


def test_middle_grey_lands_on_118_and_the_reference_on_108():
    assert E.srgb_codes(F(0.18)) == 118
    assert E.quantise(F(0.18)) == 108
    assert E.encode(flat(0.18), E.REFERENCE)[0, 0, 0] == 108
    codes = E.encode(flat(0.18), E.SRGB, True)
    assert set(np.unique(codes)) <= {117, 118, 119} and E.L[117] < F(0.18) < E.L[119]


def test_codes_are_monotone_over_a_sweep():
    rng = np.random.default_rng(20240607)
    x = np.sort(np.concatenate([rng.random(20000).astype(F) * F(1.25), E.M, E.L, np.nextafter(E.M, F(0)), np.nextafter(E.M, F(2))]))
    assert (np.diff(E.srgb_codes(x).astype(int)) >= 0).all()
    assert E.srgb_codes(x).min() == 0 and E.srgb_codes(x).max() == 255
    for t in (F(0.5 / 64), F(31.5 / 64), F(63.5 / 64)):  # at one threshold the dithered code is monotone in x too
        assert (np.diff(E.dither_codes(x, t).astype(int)) >= 0).all()
    # the thresholds are where the code steps: M[c] gives c, the binary32 before it c - 1
    assert (E.srgb_codes(E.M) == np.arange(1, 256)).all() and (E.srgb_codes(np.nextafter(E.M, F(0))) == np.arange(255)).all()


def test_specials_give_the_stated_codes():
    sub = F(1e-45)
    x = np.array([np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, -1.0, -1e-30, sub, F(2.0 ** -126), 1.0, np.nextafter(F(1), F(2)), 1.5, 3e38,
                  np.nextafter(F(1), F(0))], dtype=F)
    want = [0, 0, 255, 0, 0, 0, 0, 0, 0, 0, 255, 255, 255, 255, 255]
    assert list(E.srgb_codes(x)) == want
    for t in (F(0.5 / 64), F(63.5 / 64)):
        got = list(E.dither_codes(x, t))
        assert got[:-1] == want[:-1], (t, got)
        assert got[-1] in (254, 255)
    assert E.dither_codes(np.nextafter(F(1), F(0)), F(0.5 / 64)) == 255 and E.dither_codes(E.L[254], F(0.5 / 64)) == 254
    assert list(E.quantise(np.array([np.nan, np.inf, -np.inf, -0.0, -1.0, 1.0, sub], dtype=F))) == [0, 255, 0, 0, 0, 255, 0]
    assert E.dither_codes(sub, F(0.5 / 64)) == 0  # f = sub / L[1] is far below the smallest t


@pytest.mark.parametrize("c", [0, 1, 10, 11, 128, 254])
def test_a_flat_patch_dithers_to_its_own_mean(c):
    """A property of the definition, not a measured bound: of the 64 thresholds (k + 0.5) / 64 exactly #{t <= f} lie at or below f, those
    pixels get c + 1, and the mean of the decoded levels then differs from x by at most one 64th of the step."""
    lo, hi = np.float64(E.L[c]), np.float64(E.L[c + 1])
    t64 = E.thresholds(8, 8).astype(np.float64).ravel()
    for i in range(32):
        x = F(lo + (hi - lo) * (i + 0.37) / 32)
        assert E.L[c] <= x < E.L[c + 1]
        f = F(F(x - E.L[c]) / F(E.L[c + 1] - E.L[c]))
        for phase in ((0, 0), (5, -2)):
            codes = E.encode(flat(x), E.SRGB, True, phase)
            assert set(np.unique(codes)) <= {c, c + 1}
            assert (codes[:, :, 0] == codes[:, :, 1]).all() and (codes[:, :, 0] == codes[:, :, 2]).all()  # one t per pixel: greys stay neutral
            up = int((codes[:, :, 0] == c + 1).sum())
            assert up == int((t64 <= np.float64(f)).sum()), (i, phase)
            mean = E.L.astype(np.float64)[codes[:, :, 0]].mean()
            assert abs(mean - np.float64(x)) <= (hi - lo) / 64, (i, phase, mean, x)


# ---- hosts ------------------------------------------------------------------------------------------------------------------------------

def png_chunks(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, out = 8, []
    while at < len(data):
        n = struct.unpack(">I", data[at:at + 4])[0]
        out.append((data[at + 4:at + 8], data[at + 8:at + 8 + n]))
        at += 12 + n
    return out


def old_write_png(path, rgb8):
    """The writer as it stood before the option, verbatim."""
    import zlib

    rgb8 = np.ascontiguousarray(rgb8, dtype=np.uint8)
    h, w, c = rgb8.shape
    raw = np.concatenate([np.zeros((h, 1), dtype=np.uint8), rgb8.reshape(h, w * 3)], axis=1).tobytes()

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)))
        f.write(chunk(b"IDAT", zlib.compress(raw, 6)))
        f.write(chunk(b"IEND", b""))


def test_write_png_tags_srgb_only_when_told_to(tmp_path):
    from PIL import Image

    from path_tracer_amd.png import write_png

    rgb8 = np.random.default_rng(7).integers(0, 256, (13, 17, 3), dtype=np.uint8)
    write_png(str(tmp_path / "plain.png"), rgb8)
    write_png(str(tmp_path / "false.png"), rgb8, srgb=False)
    old_write_png(str(tmp_path / "old.png"), rgb8)
    assert (tmp_path / "plain.png").read_bytes() == (tmp_path / "old.png").read_bytes() == (tmp_path / "false.png").read_bytes()
    write_png(str(tmp_path / "srgb.png"), rgb8, srgb=True)
    tags = [t for t, _ in png_chunks((tmp_path / "srgb.png").read_bytes())]
    assert tags == [b"IHDR", b"sRGB", b"gAMA", b"IDAT", b"IEND"]
    assert dict(png_chunks((tmp_path / "srgb.png").read_bytes()))[b"sRGB"] == b"\x00"
    assert dict(png_chunks((tmp_path / "srgb.png").read_bytes()))[b"gAMA"] == struct.pack(">I", 45455)
    with Image.open(tmp_path / "srgb.png") as im:
        im.load()
        assert im.info.get("srgb") == 0 and abs(im.info.get("gamma") - 0.45455) < 1e-9
        assert (np.asarray(im) == rgb8).all()
    with Image.open(tmp_path / "plain.png") as im:
        im.load()
        assert "srgb" not in im.info and "gamma" not in im.info
        assert (np.asarray(im) == rgb8).all()


def test_the_cpp_writer_tags_srgb_only_when_told_to(tmp_path):
    from PIL import Image

    src = tmp_path / "w.cpp"
    src.write_text('#include "pt/image_io.hpp"\n#include <vector>\nint main(int, char** v) {\n  std::vector<uint8_t> p(13 * 17 * 3);\n'
                   '  for (size_t i = 0; i < p.size(); i++) p[i] = (uint8_t)(i * 7);\n'
                   '  return pt::image_io::write_png(v[1], p.data(), 17, 13) && pt::image_io::write_png(v[2], p.data(), 17, 13, false) &&\n'
                   '         pt::image_io::write_png(v[3], p.data(), 17, 13, true) ? 0 : 1;\n}\n')
    exe = tmp_path / "w"
    subprocess.run(["g++", "-std=c++20", "-O1", f"-I{ROOT / 'path_tracer_amd' / 'include'}", str(src), "-o", str(exe)], check=True)
    names = [str(tmp_path / n) for n in ("a.png", "b.png", "c.png")]
    subprocess.run([str(exe), *names], check=True, timeout=60)
    a, b, c = (Path(n).read_bytes() for n in names)
    assert a == b and [t for t, _ in png_chunks(a)] == [b"IHDR", b"IDAT", b"IEND"]
    assert [t for t, _ in png_chunks(c)] == [b"IHDR", b"sRGB", b"gAMA", b"IDAT", b"IEND"]
    want = (np.arange(13 * 17 * 3) * 7).astype(np.uint8).reshape(13, 17, 3)
    with Image.open(names[2]) as im:
        im.load()
        assert im.info.get("srgb") == 0 and abs(im.info.get("gamma") - 0.45455) < 1e-9 and (np.asarray(im) == want).all()
    # the untagged file is the tagged one without the two chunks
    assert a == c.replace(c[33:33 + 13 + 16], b"", 1)


def cli(*args):
    return subprocess.run([sys.executable, "-m", "path_tracer_amd", *args], cwd=ROOT, capture_output=True, text=True, timeout=120)


def test_cli_lists_the_options_and_rejects_bad_combinations_without_a_gpu():
    p = cli("--help")
    assert p.returncode == 0 and "--encode" in p.stdout and "--dither" in p.stdout and "srgb" in p.stdout
    for args, message in ((["--dither", "--display-out", "d.png"], "--dither needs --encode srgb"),
                          (["--encode", "srgb"], "--encode and --dither need --display-out or --frames-dir"),
                          (["--encode", "srgb", "--dither"], "--encode and --dither need --display-out or --frames-dir"),
                          (["--encode", "rec709", "--display-out", "d.png"], "invalid choice")):
        p = cli(*args)
        assert p.returncode == 2 and message in p.stderr, (args, p.stderr)


def test_python_hosts_take_the_keyword():
    import inspect

    from path_tracer_amd import render as R

    sig = inspect.signature(R.encode)
    assert list(sig.parameters)[:5] == ["linear", "transfer", "dither", "phase", "out"]
    assert (sig.parameters["transfer"].default, sig.parameters["dither"].default, sig.parameters["phase"].default) == ("srgb", False, (0, 0))
    for fn in (R.Display.apply, R.display, R.Accumulator.display, R.render_temporal):
        assert inspect.signature(fn).parameters["encode"].default is None, fn
    assert R._encode_kw(None, "x") is None and R._encode_kw("srgb", "x") == {} and R._encode_kw(dict(dither=True), "x") == dict(dither=True)
    with pytest.raises(TypeError):
        R._encode_kw(dict(gamma=2.2), "x")
    with pytest.raises(TypeError):
        R._encode_kw("rec709", "x")


def test_the_facades_program_compiles(tmp_path, lib):
    libdir = ROOT / "path_tracer_amd"
    exe = tmp_path / "encode_main"
    subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{libdir / 'include'}",
                    str(ROOT / "tests" / "cpp" / "encode_main.cpp"), "-o", str(exe), f"-L{libdir}", "-lpt_render", "-L/opt/rocm/lib",
                    "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "usage: encode_main" in p.stderr

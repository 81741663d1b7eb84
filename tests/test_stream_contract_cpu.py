"""CPU tests of the stream contract's table (tests/stream_contract.py: CONTRACT) against include/pt_render.h: the table has a row for
exactly the exported functions whose prototype takes a `void* stream`, and the header's comment on each of them says what the table
says — "asynchronous on `stream`" or "synchronises `stream`".  What the library does about it is tests/test_gpu_stream_order.py."""
import re
from pathlib import Path

from path_tracer_amd import abi
from stream_contract import CONTRACT, contract_functions

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "pt_render.h"
ASYNC = re.compile(r"asynchronous on `stream`", re.I)
SYNC = re.compile(r"\bsynchronis\w* `stream`", re.I)
NEAR = 120  # characters of a banner comment before the phrase in which the function must be named
PROTO = re.compile(r"^(?:extern\s+)?(?:int|void|int32_t|int64_t|uint32_t|const char\*)\s+(pt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", re.M)


def stream_prototypes():
    """{function: offset of its prototype in the header} for the prototypes with a `void* stream` parameter (comments blanked in place, so
    that offsets are the header's)."""
    text = HEADER.read_text()
    code = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), text, flags=re.S)
    return text, {m.group(1): m.start() for m in PROTO.finditer(code) if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2))}


def words(comment):
    return re.sub(r"\s+", " ", re.sub(r"^\s*\*", " ", comment, flags=re.M))


def comments_of(text, at):
    """(the comment above the prototype at `at`, or above the run of prototypes it stands in — "" if anything else stands between —, the
    banner comment of its section)."""
    found = list(re.finditer(r"/\*(?:(?!\*/).)*\*/", text[:at], re.S))
    own = words(found[-1].group(0)) if found and PROTO.sub("", text[found[-1].end():at]).strip() == "" else ""
    banners = [c for c in found if c.group(0).startswith("/* ----")]
    return own, words(banners[-1].group(0)) if banners else ""


def test_the_table_has_exactly_the_prototypes_that_take_a_stream():
    _, protos = stream_prototypes()
    assert len(protos) >= 28
    assert contract_functions() == set(protos), sorted(contract_functions() ^ set(protos))
    assert set(CONTRACT.values()) == {"async", "sync"}
    assert [k for k in CONTRACT if "+" in k] == ["pt_adaptive_window+mask"] and CONTRACT["pt_adaptive_window"] == "async"
    for name in protos:  # and abi.py passes each of them a stream: a pointer as the last argument but for pt_render_timed's kernel_ms
        args = abi.SIGNATURES[name][1]
        assert abi.C.c_void_p in args[-2:], name


def test_every_comment_states_what_the_table_says():
    """The comment directly above the prototype decides where it says either.  A prototype whose comment says neither may lean on its
    section's banner comment only where the banner NAMES it within the NEAR characters that lead up to "asynchronous on `stream`"
    (pt_temporal_push; the display section's "pt_display_meter, pt_display_set_exposure, pt_display_reset and pt_display_apply are
    asynchronous on `stream`"): a sentence about another function, or about none, does not speak for it."""
    text, protos = stream_prototypes()
    for row, want in CONTRACT.items():
        name = row.split("+")[0]
        own, banner = comments_of(text, protos[name])
        if name == "pt_adaptive_window":  # one comment, both rows: asynchronous without a mask, synchronising with one
            assert ASYNC.search(own) and SYNC.search(own) and "mask" in own, own
            continue
        a, s = bool(ASYNC.search(own)), bool(SYNC.search(own))
        if a or s:
            assert (a, s) == (want == "async", want == "sync"), f"{row}: the table says {want}, its comment says: {own}"
        else:  # the banner counts only where it names this function in the words that lead up to the phrase, and only for an asynchronous row
            named = any(re.search(rf"\b{name}\b", banner[max(0, m.start() - NEAR):m.start()]) for m in ASYNC.finditer(banner))
            assert want == "async" and named, f"{row}: the table says {want}; neither its own comment nor a sentence of its section's that names it says so"

"""The C entry points of the sub-receivers on the pipelined feed (ssdr_set_feed_subrx, ssdr_feed_subrx_play, ssdr_feed_collect_subrx):
the declarations, the struct against the header, the argument errors that need no ctx.  The rules of a live ctx are in
tests/test_gpu_feed_subrx.py."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ssdr_set_feed_subrx", "ssdr_get_feed_subrx", "ssdr_feed_subrx_play", "ssdr_feed_collect_subrx")


@pytest.fixture(scope="module")
def L():
    from supersdr_amd import _lib
    return _lib


def test_the_declarations_are_in_the_header_and_the_library(L):
    src = open(os.path.join(ROOT, "include", "ssdr.h")).read()
    for decl in ("int ssdr_set_feed_subrx(ssdr_ctx *ctx, int on);", "int ssdr_get_feed_subrx(ssdr_ctx *ctx, int *on);",
                 "int ssdr_feed_subrx_play(ssdr_ctx *ctx, const ssdr_play_chan *chans, uint32_t count);",
                 "int ssdr_feed_collect_subrx(ssdr_ctx *ctx, ssdr_feed_subrx *out);"):
        assert decl in src, decl
    for name in NAMES:
        assert hasattr(L.lib, name) and name in L.EXPORTS, name
    assert "#define SSDR_FEED_LISTEN 8u" in src and "SSDR_FEED_SUB" not in src       # a switch of the ctx, not a flag of the feed


def test_the_struct_is_the_headers(L):
    src = open(os.path.join(ROOT, "include", "ssdr.h")).read()
    decl = src[src.index("typedef struct ssdr_feed_subrx {"):src.index("} ssdr_feed_subrx;")]
    fields = re.findall(r"^\s+(?:const )?(\w+) (\*?)(\w+);", decl, re.M)
    assert [n for _, _, n in fields] == [n for n, _ in L.FeedSubRx._fields_]         # the header's fields in the header's order
    ctype = {"uint32_t": C.c_uint32, "int16_t": C.c_int16, "float": C.c_float, "uint8_t": C.c_uint8, "ssdr_subrx": L.SubRx,
             "ssdr_rx_stages": L.RxStages}
    for (t, star, n), (_, bound) in zip(fields, L.FeedSubRx._fields_):
        assert bound is (C.POINTER(ctype[t]) if star else ctype[t]), n
    size = 2 * 4 + 10 * C.sizeof(C.c_void_p)
    assert C.sizeof(L.FeedSubRx) == size == 88 and "/* 88 B */" in src[src.index("} ssdr_feed_subrx;"):][:80]
    assert L.FeedSubRx.list.offset == 8 and L.FeedSubRx.play.offset == 80


def test_null_arguments(L):
    lib, on, out = L.lib, C.c_int(7), L.FeedSubRx()
    assert lib.ssdr_set_feed_subrx(None, 1) == L.EINVAL
    assert lib.ssdr_get_feed_subrx(None, C.byref(on)) == L.EINVAL and on.value == 7
    assert lib.ssdr_feed_subrx_play(None, None, 0) == L.EINVAL
    assert lib.ssdr_feed_collect_subrx(None, C.byref(out)) == L.EINVAL
    assert lib.ssdr_feed_collect_subrx(None, None) == L.EINVAL

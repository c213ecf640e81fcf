"""The test-only library of tests/internal_shim.py on the build machine (no GPU): it compiles against the internal headers (a
forwarder whose parameter list differs from its declaration fails that compile), exports every kwst_* name the GPU tests use,
leaves libkws_hip.so alone, and kwst_gather_strided_rows - pure host code - takes exactly the shortcut gathers the residual
programs' planner builds whose rows have a uniform pitch, and refuses the odd lengths where clip borders break it."""
import ctypes
import os
import shutil
import subprocess

import pytest

import internal_shim

pytestmark = pytest.mark.skipif(not os.path.exists(internal_shim.HIPCC), reason="no hipcc")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = internal_shim.build(str(tmp_path_factory.mktemp("kwst")))
    return so, internal_shim.load(so)


def test_shim_exports_every_forwarder(shim):
    so, _ = shim
    syms = internal_shim.exported_symbols(so)
    missing = [n for n in list(internal_shim.KWST_SIGNATURES) + internal_shim.PUBLIC if n not in syms]
    assert not missing, missing
    # nothing else of the shim leaks: its only exports beyond the library's public C ABI are the forwarders
    assert sorted(n for n in syms if n.startswith("kwst_")) == sorted(internal_shim.KWST_SIGNATURES)


def test_forwarder_with_a_wrong_signature_fails_the_build(tmp_path):
    """The static_assert of KWST_FORWARD, not a cast, decides: a forwarder that drops the stream of its declaration must not
    compile."""
    src = open(internal_shim.SHIM_SRC).read()
    bad = src.replace("(const float* a, const float* b, float* out, int64_t n, hipStream_t st), (a, b, out, n, st)",
                      "(const float* a, const float* b, float* out, int n, hipStream_t st), (a, b, out, n, st)")
    assert bad != src
    path = tmp_path / "bad_shim.cpp"
    path.write_text(bad)
    r = subprocess.run([internal_shim.HIPCC, "-std=c++17", "--offload-arch=gfx950", "-fsyntax-only", "-I", internal_shim.CSRC,
                        "-x", "hip", str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "does not match the declaration of kws_add_f32" in r.stderr


def test_tail_struct_mirrors_match_the_library(shim):
    """The ctypes mirrors of the tails' argument structs have the size and last-member offset the library was compiled with: a
    member added, removed or retyped in csrc/internal.h fails here, on the build machine."""
    _, lib = shim
    mine = [(ctypes.sizeof(cls), getattr(cls, last).offset) for cls, last in internal_shim.TAIL_STRUCTS]
    assert mine == internal_shim.tail_struct_layout(lib)
    # the mirrors' member order, member for member, against the header's text
    src = open(os.path.join(internal_shim.CSRC, "internal.h")).read()
    for cls, cname in zip([c for c, _ in internal_shim.TAIL_STRUCTS], ["kws_ts_tail_args", "kws_tail_post_args", "kws_flat_tail_args"]):
        body = src.split("struct %s {" % cname)[1].split("};")[0]
        names = []
        for decl in body.split(";"):
            decl = " ".join(l.split("//")[0] for l in decl.splitlines()).strip()
            if decl:
                names += [part.split()[-1].lstrip("*") for part in decl.split(",")]
        assert names == [f[0] for f in cls._fields_], cname


def test_gbn_struct_mirrors_match_the_library(shim):
    """kws_gbn_cols / kws_gbn_refs (csrc/internal.h) against their ctypes mirrors: size, last-member offset, member order."""
    _, lib = shim
    mine = [(ctypes.sizeof(cls), getattr(cls, last).offset) for cls, last in internal_shim.GBN_STRUCTS]
    assert mine == internal_shim.gbn_struct_layout(lib)
    src = open(os.path.join(internal_shim.CSRC, "internal.h")).read()
    for (cls, _), cname in zip(internal_shim.GBN_STRUCTS, ["kws_gbn_cols", "kws_gbn_refs"]):
        body = src.split("struct %s {" % cname)[1].split("};")[0]
        names = []
        for decl in body.split(";"):
            decl = " ".join(l.split("//")[0] for l in decl.splitlines()).strip()
            if decl:
                names += [part.split()[-1].lstrip("*") for part in decl.split(",")]
        assert names == [f[0] for f in cls._fields_], cname


def _gather(d):
    g = internal_shim.Gather()
    for k, v in d.items():
        setattr(g, k, v)
    return g


def test_gather_strided_rows_on_the_planners_shortcuts(shim):
    _, lib = shim
    seen_even = seen_odd = 0
    for name in internal_shim.PROGRAMS:
        blocks = internal_shim.planner_blocks(lib, name)
        assert blocks, name
        for blk in blocks:
            if "gather" not in blk:
                continue
            d = blk["gather"]
            lda = ctypes.c_int(-1)
            ok = lib.kwst_gather_strided_rows(ctypes.byref(_gather(d)), ctypes.byref(lda))
            if blk["L"] % 2 == 0:
                # an even input: row (b, t) = input row 2 (b L_out + t) of the [B L, cin] matrix, a pitch of 2 cin floats
                assert ok and lda.value == 2 * blk["cin"], (name, blk)
                seen_even += 1
            else:
                # an odd input (r06: "odd lengths keep the gathered kernels"): clip b starts at row b L, not at 2 b L_out
                assert not ok and lda.value == -1, (name, blk)
                seen_odd += 1
    assert seen_even > 0 and seen_odd > 0        # both sides of the rule occur in the programs


def test_gather_strided_rows_refusals(shim):
    _, lib = shim
    base = dict(L_out=24, cin=64, taps=1, stride_t=128, stride_j=0, base_off=0, x_len=48 * 64, x_batch_stride=48 * 64)
    lda = ctypes.c_int(0)
    assert lib.kwst_gather_strided_rows(ctypes.byref(_gather(base)), ctypes.byref(lda)) and lda.value == 128
    for change in (dict(taps=3), dict(base_off=-64), dict(stride_t=32), dict(stride_t=130, x_batch_stride=24 * 130, x_len=24 * 130),
                   dict(x_batch_stride=47 * 64, x_len=47 * 64), dict(x_len=46 * 64 + 63), dict(cin=0)):
        d = dict(base, **change)
        lda = ctypes.c_int(-1)
        assert not lib.kwst_gather_strided_rows(ctypes.byref(_gather(d)), ctypes.byref(lda)), change
        assert lda.value == -1
    assert not lib.kwst_gather_strided_rows(None, ctypes.byref(lda))


def test_libkws_hip_is_not_touched(shim):
    """The shim is linked beside the library, never into it: libkws_hip.so keeps exactly its header's exports."""
    from speech_recognition_amd import _lib
    if not os.path.exists(_lib.LIB_PATH) or shutil.which("nm") is None:
        pytest.skip("libkws_hip.so not built")
    syms = internal_shim.exported_symbols(_lib.LIB_PATH)
    assert not [n for n in syms if n.startswith("kwst_")]
    assert "kws_block_out_fwd" not in syms and "kws_reduce_slabs_batch" not in syms

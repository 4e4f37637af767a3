"""The split-K grad-weight GEMM's host side: declarations, bindings and the split / workspace arithmetic (not gpu)."""

import os
import re

import pytest

from nerf_sampling_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ns_gemm_wgrad", "ns_gemm_wgrad_splits", "ns_gemm_wgrad_workspace_bytes")
SHAPES = [(256, 256), (256, 319), (128, 283), (3, 128), (1, 256), (32, 32), (1, 63), (97, 160), (512, 512), (40, 72)]
ROWS = [1, 2, 5, 100, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 8193, 20001, 32768, 32769, 65536, 65537, 196608, 1 << 20,
        (1 << 31) - 1]


def header_text():
    text = open(os.path.join(ROOT, "include", "nerf_sampling_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_entries_and_the_bindings_match():
    text = header_text()
    for name in ENTRIES:
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in the header"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == n_args, (name, n_args, len(_lib.SIGNATURES[name][1]))
    lib = _lib.load()
    for name in ENTRIES:
        assert hasattr(lib, name)


@pytest.mark.parametrize("N,K", SHAPES)
def test_splits(N, K):
    lib = _lib.load()
    prev = 1
    for rows in ROWS:
        s = lib.ns_gemm_wgrad_splits(rows, N, K)
        assert s >= 1
        if rows <= 1024:
            assert s == 1, (rows, N, K, s)
        assert s >= prev, "the split count must not decrease with the rows"
        assert s == lib.ns_gemm_wgrad_splits(rows, N, K), "a pure function of (rows, N, K)"
        prev = s


def test_fit_batches_occupy_every_cu():
    """tiles x splits >= 256 workgroups at the field fit's 1024 x 192 batch; tiles no larger than 64 x 64 outputs"""
    lib = _lib.load()
    for N, K in ((256, 256), (256, 319)):
        tiles_at_most = ((N + 31) // 32) * ((K + 31) // 32)
        tiles_at_least = ((N + 63) // 64) * ((K + 63) // 64)
        s = lib.ns_gemm_wgrad_splits(196608, N, K)
        assert tiles_at_least * s >= 256, (N, K, s)
        assert s <= 196608 // 512 and tiles_at_most * s <= 1 << 16


@pytest.mark.parametrize("N,K", SHAPES)
def test_workspace_bytes(N, K):
    lib = _lib.load()
    prev = 0
    for rows in ROWS:
        s = lib.ns_gemm_wgrad_splits(rows, N, K)
        b = lib.ns_gemm_wgrad_workspace_bytes(rows, N, K)
        if s == 1:
            assert b == 0
        else:
            assert b >= s * N * K * 4
            assert b % 256 == 0 and b == (s * (N * K + N) * 4 + 255) // 256 * 256      # the header's formula
        assert b >= prev, "monotone in the rows"
        prev = b


def test_bad_arguments_are_reported_without_a_gpu():
    lib = _lib.load()
    one = 0x1000          # never dereferenced: validation comes first
    ok = dict(dy=one, s0=4, s1=1, x=one, sx=8, rows=16, N=4, K=8, dW=one, ldw=8, acc=0, db=None, ws=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ns_gemm_wgrad(a["dy"], a["s0"], a["s1"], a["x"], a["sx"], a["rows"], a["N"], a["K"], a["dW"], a["ldw"], a["acc"],
                                 a["db"], a["ws"], None)

    for bad in (dict(dy=None), dict(x=None), dict(dW=None), dict(rows=0), dict(rows=-1), dict(rows=1 << 31), dict(N=0),
                dict(K=0), dict(ldw=7), dict(s0=-1), dict(sx=-1), dict(acc=2), dict(rows=4096, ws=None)):
        assert call(**bad) == -1, bad
        assert b"ns_gemm_wgrad" in lib.ns_last_error()
    for bad in (dict(N=513), dict(K=513, ldw=513)):
        assert call(**bad) == -2, bad

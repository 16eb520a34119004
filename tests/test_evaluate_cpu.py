"""Host-only checks of the validation path: the beam search's workspace no longer grows by a copy of the
annotations and of Vh per hypothesis row (content attention), and the new entry points / flag are declared."""
import ctypes
import inspect

from s2s_amd import _lib
from s2s_amd._lib import lib

FLOAT = 4


def _dims(B, L, A=512, Sc=512, S=256, O=62, M=64, Kw=7, hyb=(0, 0)):
    d = _lib.s2s_attn_dims(B, L, 1, A, Sc, S, O, M, Kw, 0.0, 0.0)
    d.hybridAttendFilterSize, d.hybridAttendFeatureMaps = hyb
    return d


def _bytes(d, K, maxlen):
    n = lib.s2s_attn_beam_workspace_bytes(ctypes.byref(d), K, maxlen)
    assert n > 0
    return n


def test_beam_workspace_does_not_replicate_the_annotations():
    """A = Sc = 512, S = 256, B = 8, L = 256: going from K = 1 to K = 16 adds 15 * B hypothesis rows.  Each cost
    L * (A + Sc) = 1024 L floats when h and Vh were copied per row; with both shared only the scores, alpha,
    the chunk partials and small per-row state remain: fewer than 64 L floats per row."""
    B, L = 8, 256
    d = _dims(B, L)
    grow = _bytes(d, 16, L) - _bytes(d, 1, L)
    print(f"workspace growth K = 1 -> 16: {grow} bytes = {grow / (15 * B * L * FLOAT):.1f} floats per row and frame")
    assert grow < 15 * B * L * 64 * FLOAT


def test_replicated_arm_and_hybrid_attention_keep_a_copy_per_row():
    """The debug knob's arm and hybrid attention (alpha_{t-1} per hypothesis feeds the location features) still
    lay out one copy of h and Vh per hypothesis row: the knob is not inert, and it is restored."""
    B, L = 8, 256
    per_copy = 15 * B * L * 1024 * FLOAT
    hyb = _dims(B, L, hyb=(5, 8))
    assert _bytes(hyb, 16, L) - _bytes(hyb, 1, L) >= per_copy
    d = _dims(B, L)
    shared = _bytes(d, 16, L)
    lib.s2s_debug_beam_replicate.argtypes, lib.s2s_debug_beam_replicate.restype = [ctypes.c_int], None
    lib.s2s_debug_beam_replicate(1)
    try:
        assert _bytes(d, 16, L) - _bytes(d, 1, L) >= per_copy
    finally:
        lib.s2s_debug_beam_replicate(0)
    assert _bytes(d, 16, L) == shared


def test_new_entry_points_are_bound():
    names = {n for n, _, _ in _lib.SIGNATURES}
    assert {"s2s_attn_beam_set_maxlens", "s2s_attn_beam_search_ragged"} <= names
    assert _lib.S2S_FORWARD_ONLY == 8
    for n in ("s2s_attn_beam_set_maxlens", "s2s_attn_beam_search_ragged"):
        assert getattr(lib, n).restype is ctypes.c_int


def test_python_surface():
    import s2s_amd
    p = inspect.signature(s2s_amd.Attention.BeamSearch).parameters
    assert list(p)[1:] == ["annotations", "eos", "K", "maxseqlength", "finished", "frame_lengths", "maxseqlengths"]
    assert p["frame_lengths"].default is None and p["maxseqlengths"].default is None
    f = inspect.signature(s2s_amd.ChorowskiBaseline.forward).parameters
    assert list(f)[1:] == ["x", "labels", "frame_lengths", "label_lengths", "normalizeNLL", "stream"]
    assert f["normalizeNLL"].default is False
    e = inspect.signature(s2s_amd.ChorowskiBaseline.Evaluate).parameters
    assert list(e)[1:] == ["xs", "ys", "K", "max_batch", "eos", "token_map"]
    assert (e["K"].default, e["max_batch"].default) == (5, 32)

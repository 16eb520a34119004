"""Host-only checks of the opt-in shared-annotation beam search for hybrid attention: the new dims field is
mirrored everywhere, 0 keeps today's per-row workspace, 1 sizes the workspace as content attention's plus the
per-hypothesis alpha double buffer."""
import ctypes
import os
import re

from s2s_amd import _lib
from s2s_amd._lib import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOAT = 4
B, L = 8, 256


def _dims(hyb, share=0):
    d = _lib.s2s_attn_dims(B, L, 1, 512, 512, 256, 62, 64, 7, 0.0, 0.0)
    d.hybridAttendFilterSize, d.hybridAttendFeatureMaps = hyb
    d.beam_share_hybrid = share
    return d


def _bytes(d, K):
    n = lib.s2s_attn_beam_workspace_bytes(ctypes.byref(d), K, L)
    assert n > 0
    return n


def test_the_field_is_mirrored():
    assert _lib.s2s_attn_dims._fields_[-1] == ("beam_share_hybrid", ctypes.c_int)
    hdr = open(os.path.join(ROOT, "include", "s2s_hip.h")).read()
    body = re.search(r"typedef struct \{((?:(?!typedef).)*)\}\s*s2s_attn_dims;", hdr, re.S).group(1)
    assert re.sub(r"/\*.*?\*/", " ", body, flags=re.S).split(";")[-2].split() == ["int", "beam_share_hybrid"]
    shim = open(os.path.join(ROOT, "seq2seq-attention-asr_amd", "lua", "s2s_ffi.lua")).read()
    assert re.search(r"const int\* label_lengths; int beam_share_hybrid; \} s2s_attn_dims;", shim)
    import s2s_amd
    assert s2s_amd.Attention.share_hybrid_search is False
    assert _lib.s2s_attn_dims(1, 1, 1).beam_share_hybrid == 0


def test_off_keeps_the_replicated_workspace():
    """beam_share_hybrid = 0: a hybrid dims' workspace is what the replicated arm lays out (today's value), and on
    content attention the field changes nothing either way."""
    lib.s2s_debug_beam_replicate.argtypes, lib.s2s_debug_beam_replicate.restype = [ctypes.c_int], None
    for K in (1, 5, 16):
        off = _bytes(_dims((5, 8)), K)
        lib.s2s_debug_beam_replicate(1)
        try:
            assert _bytes(_dims((5, 8)), K) == off
            assert _bytes(_dims((5, 8), 1), K) == off  # the knob's arm replicates whatever the field says
        finally:
            lib.s2s_debug_beam_replicate(0)
        assert _bytes(_dims((5, 8)), K) == off
        assert _bytes(_dims((0, 0), 1), K) == _bytes(_dims((0, 0)), K)


def test_on_shares_the_annotations():
    """A = Sc = 512, S = 256, B = 8, L = 256, kW = 5 / 8 maps.  K = 1 -> 16 adds 15 * B rows: over content
    attention's growth a shared hybrid search adds the alpha double buffer (2 L floats per row; 2 L more allowed
    for alignment), and stays under an eighth of the 1024 L floats per row that the copies of h and Vh cost."""
    rows = 15 * B
    content = _bytes(_dims((0, 0)), 16) - _bytes(_dims((0, 0)), 1)
    repl = _bytes(_dims((5, 8)), 16) - _bytes(_dims((5, 8)), 1)
    shared = _bytes(_dims((5, 8), 1), 16) - _bytes(_dims((5, 8), 1), 1)
    print(f"growth K = 1 -> 16, floats per row and frame: content {content / (rows * L * FLOAT):.2f}, shared "
          f"hybrid {shared / (rows * L * FLOAT):.2f}, replicated hybrid {repl / (rows * L * FLOAT):.2f}; "
          f"bytes at K = 5: shared {_bytes(_dims((5, 8), 1), 5)}, replicated {_bytes(_dims((5, 8)), 5)}")
    assert shared >= content + rows * 2 * L * FLOAT  # the alpha double buffer is there
    assert shared - content <= rows * 4 * L * FLOAT
    assert shared < repl / 8

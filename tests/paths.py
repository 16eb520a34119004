"""Which kernel path ran: the library's host-side record of dispatch decisions, for the GPU tests.

The library picks a path (per-step launches, the persistent kernels, the XCD-local decoder, ...) from exact
dimensions and process-wide knobs.  A test written for one path, or comparing two paths as A/B arms, proves
nothing when the dispatch quietly sends it elsewhere, so such tests wrap their launches in `decisions()` and
assert what the launch code recorded (csrc/decisions.h: filled where the launch is issued, never recomputed).

    with decisions() as dec:
        att.forward(...)
    assert dec["dec.fwd.path"] == XCD

S2S_DEC_MODE is read once per process, so a test cannot select a decoder path through the environment once any
attention call has run; `dec_mode(m)` sets the in-process override (s2s_debug_dec_mode) and restores it.
"""
import contextlib
import ctypes

# dec.fwd.path / dec.bwd.path
STEPS, PERSIST, XCD, XCD_LSTM = 0, 1, 2, 3
# s2s_debug_dec_mode
MODE_AUTO, MODE_STEP, MODE_PERSIST = 0, 1, 2


def _lib():
    from s2s_amd import _lib
    lib = _lib.lib
    lib.s2s_debug_decisions.argtypes = [ctypes.c_int]
    lib.s2s_debug_decisions.restype = None
    lib.s2s_debug_decisions_clear.argtypes = []
    lib.s2s_debug_decisions_clear.restype = None
    lib.s2s_debug_decision.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_long)]
    lib.s2s_debug_decision.restype = ctypes.c_int
    lib.s2s_debug_dec_mode.argtypes = [ctypes.c_int]
    lib.s2s_debug_dec_mode.restype = None
    return lib


class Reader:
    """Reads the record: r[name] is the last value (KeyError when the site never ran), r.count(name) how often
    it was recorded since the record was cleared, r.get(name) the value or None.  A reader outlives its
    `decisions()` block through the snapshot taken when the block ends."""

    def __init__(self, lib):
        self._lib = lib
        self._frozen = None

    def _read(self, name):
        if self._frozen is not None:
            return self._frozen.get(name)
        v, c = ctypes.c_long(0), ctypes.c_long(0)
        if not self._lib.s2s_debug_decision(name.encode(), ctypes.byref(v), ctypes.byref(c)):
            return None
        return v.value, c.value

    def get(self, name):
        e = self._read(name)
        return None if e is None else e[0]

    def __getitem__(self, name):
        e = self._read(name)
        if e is None:
            raise KeyError(f"decision {name!r} was not recorded: its launch site did not run")
        return e[0]

    def count(self, name):
        e = self._read(name)
        return 0 if e is None else e[1]

    def _freeze(self, names):
        snap = {}
        for n in names:
            e = self._read(n)
            if e is not None:
                snap[n] = e
        self._frozen = snap


# every name the library records (csrc: attn.hip and its beam.inc, gru.hip, gru_persist.hip, lstm.hip,
# lstm_persist.hip, model_step.cpp), for the snapshot a reader keeps after its block
NAMES = (
    "dec.fwd.path", "dec.bwd.path", "dec.var", "dec.U", "dec.nchains", "dec.XLC", "dec.NCH", "dec.res",
    "dec.persist_res", "dec.allow_local", "dec.merged_head", "dec.head_bwd_fused", "dec.head_sums_slabs", "dec.r4",
    "dec.pf", "gru.fwd.path", "gru.bwd.path", "gru.fused_xproj", "gru.fused_dy", "gru.xp_split", "gru.xp_group",
    "gru.local", "gru.ring", "lstm.fwd.path", "lstm.bwd.path", "step.bptt_wgrad_in", "step.fuse_dh",
    "step.sync_handover",
)


@contextlib.contextmanager
def decisions():
    """Enable and clear the record, yield a reader, disable the record again."""
    lib = _lib()
    reader = Reader(lib)
    lib.s2s_debug_decisions_clear()
    lib.s2s_debug_decisions(1)
    try:
        yield reader
    finally:
        lib.s2s_debug_decisions(0)
        reader._freeze(NAMES)
        lib.s2s_debug_decisions_clear()


@contextlib.contextmanager
def dec_mode(m):
    """Force the decoder path in this process (MODE_STEP / MODE_PERSIST; MODE_AUTO: the dispatch's own choice
    whatever the environment says), back to the environment's afterwards."""
    lib = _lib()
    lib.s2s_debug_dec_mode(m)
    try:
        yield
    finally:
        lib.s2s_debug_dec_mode(-1)


def took(reader, name, value):
    """Assert that decision `name` was recorded at least once and last took `value`."""
    assert reader.count(name) > 0, f"{name} was not recorded: the launch that decides it did not run"
    assert reader[name] == value, f"{name} = {reader[name]}, expected {value}"


def differ(a, b, name):
    """Assert that two arms of an A/B test differ in decision `name` (an inert knob makes the test x == x)."""
    assert a.count(name) > 0 and b.count(name) > 0, f"{name} was not recorded in both arms"
    assert a[name] != b[name], f"arms do not differ: {name} = {a[name]} in both"

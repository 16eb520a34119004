"""Batch assembly on the device (s2s_pad_batch / s2s_pad_labels), DeviceLengths, PackedUtterances and the
front-ends' output lengths.

GPU: the two kernels bitwise against a torch restatement -- dst is pre-filled with NaN (unwritten padding shows), a
64-element canary behind dst must stay untouched, lengths above Lmax clamp.  The cases cover the scalar path
(F % 4 != 0, or an utterance that does not start on 16 bytes), the float4 path, both in one launch, several planes
(the VGG layout) and a single element.  CPU: the host-side argument checks, which run before any device call.
"""
import ctypes

import numpy as np
import pytest
import torch

import s2s_amd
from s2s_amd import data
from s2s_amd.nn import DeviceLengths, S2SArgumentError

CANARY = 64


def _pack(utts, gaps):
    """Flat source with gaps[b] unused floats in front of utterance b -> (flat, element offsets)."""
    parts, offs, pos = [], [], 0
    for u, g in zip(utts, gaps):
        parts.append(np.full(g, 777.0, np.float32))
        pos += g
        offs.append(pos)
        parts.append(u.reshape(-1))
        pos += u.size
    return np.concatenate(parts), np.asarray(offs, np.int64)


def _run_pad_batch(B, C, Lmax, F, lengths, gaps, seed):
    from s2s_amd.nn import check, dptr, get_context, lib, stream_ptr
    rng = np.random.default_rng(seed)
    utts = [rng.standard_normal((C, L, F)).astype(np.float32) for L in lengths]
    flat, offs = _pack(utts, gaps)
    src = torch.tensor(flat, device="cuda")
    n = B * C * Lmax * F
    buf = torch.full((n + CANARY,), float("nan"), device="cuda")
    buf[n:] = 123.5
    offd, lend = torch.tensor(offs, device="cuda"), torch.tensor(lengths, dtype=torch.int32, device="cuda")
    check(lib.s2s_pad_batch(get_context(0).handle, stream_ptr(), B, C, Lmax, F, dptr(src), dptr(offd), dptr(lend),
                            dptr(buf)))
    torch.cuda.synchronize()
    want = torch.zeros((B, C, Lmax, F))
    for b, u in enumerate(utts):
        k = min(lengths[b], Lmax)
        want[b, :, :k] = torch.from_numpy(u[:, :k])
    got = buf[:n].cpu().view(B, C, Lmax, F)
    assert torch.equal(got, want)  # (NaN anywhere fails: NaN != 0)
    assert torch.equal(buf[n:].cpu(), torch.full((CANARY,), 123.5))
    return src, offs


PAD_CASES = {
    "one_element_row": (1, 1, 1, 3, [1], [0]),
    "scalar_unaligned_offsets": (5, 1, 9, 3, [9, 1, 4, 8, 9], [1, 2, 2, 2, 1]),
    "float4_F20": (4, 1, 17, 20, [17, 3, 16, 1], [0, 0, 0, 0]),
    "vgg_planes": (3, 3, 12, 16, [12, 5, 1], [0, 0, 0]),
    "mixed_alignment_F8": (4, 1, 6, 8, [6, 2, 5, 3], [0, 1, 3, 2]),  # utterances 0 and 2 start on 16 bytes
    "clamped": (3, 2, 5, 8, [9, 5, 7], [0, 0, 2]),
    "clamped_scalar": (2, 1, 4, 5, [6, 2], [0, 3]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PAD_CASES))
def test_pad_batch_bitwise(name):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    B, C, Lmax, F, lengths, gaps = PAD_CASES[name]
    _, offs = _run_pad_batch(B, C, Lmax, F, lengths, gaps, seed=len(name))
    if name == "scalar_unaligned_offsets":
        assert all(o % 4 for o in offs)
    if name == "mixed_alignment_F8":
        assert [o % 4 == 0 for o in offs] == [True, False, True, False]


@pytest.mark.gpu
@pytest.mark.parametrize("B,Tmax,lengths", [(1, 1, [1]), (5, 7, [7, 1, 4, 7, 2]), (3, 4, [6, 4, 9])])
def test_pad_labels_bitwise(B, Tmax, lengths):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from s2s_amd.nn import check, dptr, get_context, lib, stream_ptr
    rng = np.random.default_rng(B + Tmax)
    seqs = [rng.integers(1, 60, T).astype(np.int32) for T in lengths]
    offs = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
    src = torch.tensor(np.concatenate(seqs), device="cuda")
    buf = torch.full((B * Tmax + CANARY,), -7, dtype=torch.int32, device="cuda")
    offd, lend = torch.tensor(offs, device="cuda"), torch.tensor(lengths, dtype=torch.int32, device="cuda")
    check(lib.s2s_pad_labels(get_context(0).handle, stream_ptr(), B, Tmax, dptr(src), dptr(offd), dptr(lend),
                             dptr(buf)))
    torch.cuda.synchronize()
    want = torch.zeros((B, Tmax), dtype=torch.int32)
    for b, q in enumerate(seqs):
        k = min(lengths[b], Tmax)
        want[b, :k] = torch.from_numpy(q[:k])
    assert torch.equal(buf[:B * Tmax].cpu().view(B, Tmax), want)
    assert torch.equal(buf[B * Tmax:].cpu(), torch.full((CANARY,), -7, dtype=torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("planes", [False, True])
def test_packed_utterances_batch_and_refill(planes):
    """batch() equals the host-side padding; batch(out=...) refills the same buffers and DeviceLengths in place."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    rng = np.random.default_rng(5)
    Ls, Ts, F = [7, 3, 9, 4, 8, 9], [2, 5, 1, 3, 4, 5], 6
    xs = [rng.standard_normal((3, L, F) if planes else (L, F)).astype(np.float32) for L in Ls]
    ys = [rng.integers(0, 30, T) for T in Ts]
    pk = data.PackedUtterances(xs, ys)

    def want(idx, Lmax, Tmax):
        x = np.zeros((len(idx), 3, Lmax, F) if planes else (len(idx), Lmax, F), np.float32)
        y = np.zeros((len(idx), Tmax), np.int32)
        for j, i in enumerate(idx):
            x[j, ..., :Ls[i], :] = xs[i]
            y[j, :Ts[i]] = ys[i]
        return x, y

    out = pk.batch([2, 0, 5], 12, 8)
    x, y, fl, tl, gL, gT = out
    wx, wy = want([2, 0, 5], 12, 8)
    assert np.array_equal(x.cpu().numpy(), wx) and np.array_equal(y.cpu().numpy(), wy)
    assert (gL, gT) == ([9, 7, 9], [1, 2, 5]) and fl.tensor.tolist() == gL and tl.tensor.tolist() == gT
    ptrs = (x.data_ptr(), y.data_ptr(), fl.tensor.data_ptr(), tl.tensor.data_ptr())
    x2, y2, fl2, tl2, gL, gT = pk.batch([1, 3, 4], out=out)
    assert (x2.data_ptr(), y2.data_ptr(), fl2.tensor.data_ptr(), tl2.tensor.data_ptr()) == ptrs
    wx, wy = want([1, 3, 4], 12, 8)
    assert np.array_equal(x2.cpu().numpy(), wx) and np.array_equal(y2.cpu().numpy(), wy)
    assert fl2.tensor.tolist() == [3, 4, 8] and tl2.tensor.tolist() == [5, 3, 4]
    x3 = pk.batch([0, 1])[0]  # defaults: the batch's own longest
    assert x3.shape[-2] == 7
    with pytest.raises(S2SArgumentError):
        pk.batch([0, 1], out=out)  # another batch size than out's
    with pytest.raises(S2SArgumentError):
        pk.batch([0, 1, 2], 13, 8, out=out)  # another padded shape than out's


@pytest.mark.gpu
def test_device_lengths_fill_keeps_pointer_and_derived_follow():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    enc = s2s_amd.VGGEncoder(16, 16, 16)
    fl = DeviceLengths([40, 29, 10], 40)
    lp = fl.derive("vgg", enc.out_lengths, 16)
    assert lp is fl.derive("vgg", enc.out_lengths, 16)
    p, q = fl.tensor.data_ptr(), lp.tensor.data_ptr()
    assert lp.tensor.tolist() == [16, 10, 1]
    fl.fill_([12, 40, 33])
    assert (fl.tensor.data_ptr(), lp.tensor.data_ptr()) == (p, q)
    assert fl.tensor.tolist() == [12, 40, 33] and lp.tensor.tolist() == [2, 16, 12]
    with pytest.raises(S2SArgumentError):
        fl.fill_([12, 40, 9])  # valid itself, but the derived front-end lengths refuse it
    assert fl.tensor.tolist() == [12, 40, 33] and lp.tensor.tolist() == [2, 16, 12]  # nothing was written


# ------------------------------------------------------------------------------------------------ CPU

def test_device_lengths_argument_checks():
    ok = DeviceLengths([3, 1, 5], 5, device="cpu")
    assert ok.tensor.tolist() == [3, 1, 5] and ok.tensor.dtype == torch.int32 and (ok.n, ok.maxlen) == (3, 5)
    for bad in ([3, 0, 5], [3, 6, 5], [-1, 2, 2], []):
        with pytest.raises(S2SArgumentError):
            DeviceLengths(bad, 5)  # refused on the host, before any device is touched
    for bad in ([3, 1], [3, 1, 5, 2], [3, 0, 5], [3, 6, 5]):
        with pytest.raises(S2SArgumentError):
            ok.fill_(bad)
    assert ok.tensor.tolist() == [3, 1, 5]
    p = ok.tensor.data_ptr()
    assert ok.fill_([5, 5, 1]) is ok and ok.tensor.tolist() == [5, 5, 1] and ok.tensor.data_ptr() == p
    assert ok.ptr(3, 5) == p and ok.ptr(3, 9) == p
    with pytest.raises(S2SArgumentError):
        ok.ptr(4, 5)  # another batch size
    with pytest.raises(S2SArgumentError):
        ok.ptr(3, 4)  # values may exceed a batch padded to 4


def test_packed_utterances_argument_checks():
    x = [np.zeros((4, 3), np.float32), np.zeros((2, 3), np.float32)]
    with pytest.raises(S2SArgumentError):
        data.PackedUtterances(x, [[1, 2]])  # wrong count
    with pytest.raises(S2SArgumentError):
        data.PackedUtterances([], [])
    with pytest.raises(S2SArgumentError):
        data.PackedUtterances([x[0], np.zeros((0, 3), np.float32)], [[1], [2]])  # 0 frames
    with pytest.raises(S2SArgumentError):
        data.PackedUtterances(x, [[1], []])  # 0 labels
    with pytest.raises(S2SArgumentError):
        data.PackedUtterances([x[0], np.zeros((2, 4), np.float32)], [[1], [2]])  # another frame size
    with pytest.raises(S2SArgumentError):
        data.PackedUtterances([x[0], np.zeros((1, 2, 3), np.float32)], [[1], [2]])  # mixed layouts
    pk = data.PackedUtterances(x, [[1, 2, 3], [4]])
    assert (pk.Ls, pk.Ts, pk.C, pk.F, len(pk)) == ([4, 2], [3, 1], 1, 3, 2)
    for kw in (dict(Lmax=3), dict(Tmax=2)):  # above maxlen: refused on the host, before the upload
        with pytest.raises(S2SArgumentError):
            pk.batch([0, 1], **kw)
    with pytest.raises(S2SArgumentError):
        pk.batch([0, 2])
    with pytest.raises(S2SArgumentError):
        pk.batch([])


def test_front_end_output_lengths():
    conv = s2s_amd.ConvBiLSTMEncoder(20, 32, 16)
    assert conv.out_lengths([22, 23, 60]) == [1, 1, 5]
    assert conv.out_lengths([38, 41, 44]) == [3, 3, 3]  # one L' at three raw lengths (30..37 give 2)
    assert conv.out_lengths([]) == []
    vgg = s2s_amd.VGGEncoder(16, 16, 16)
    assert vgg.out_lengths([10, 11, 40]) == [1, 1, 16]
    # the closed forms agree with running the stages
    for L in range(22, 200):
        n = L
        for _ in range(3):
            n = (n - 2) // 2
        assert conv.out_lengths([L]) == [n]
    for L in range(10, 100):
        assert vgg.out_lengths([L]) == [((L - 4) - 4) // 2]


def test_short_utterances_are_refused_with_the_minimum():
    conv = s2s_amd.ConvBiLSTMEncoder(20, 32, 16)
    with pytest.raises(S2SArgumentError, match="22"):
        conv.out_lengths([60, 21])
    vgg = s2s_amd.VGGEncoder(16, 16, 16)
    with pytest.raises(S2SArgumentError, match="10"):
        vgg.out_lengths([9])


def test_pad_batch_refuses_null_and_empty_arguments():
    """The C ABI reports instead of launching (no GPU needed: the checks come first)."""
    from s2s_amd._lib import lib
    assert lib.s2s_pad_batch(None, None, 1, 1, 1, 1, None, None, None, None) != 0
    assert lib.s2s_pad_labels(None, None, 1, 1, None, None, None, None) != 0
    assert ctypes.c_char_p(lib.s2s_last_error()).value

"""nn.Module mirrors of the encoder front-ends over libs2s_hip.so.

Operators (Torch7 nn semantics, include/s2s_hip.h "encoder front-ends"): TemporalConvolution,
TemporalMaxPooling, ReLU, SpatialConvolutionMM, SpatialMaxPooling, Transpose2 and a Sequential
container; and the two encoders the reference builds from them:
  * ConvBiLSTMEncoder -- timit/timit.lua:108-125 (conv stack shared by both LSTM directions);
  * VGGEncoder        -- librispeech/model_vgg.lua:23-51.
A convolution built with relu=True is the reference's `conv -> nn.ReLU()` pair fused (the ReLU runs in
the GEMM epilogue; its backward masks by the conv output).  Gradients accumulate; backward returns
gradInput (None for a module built with need_gradInput=False: the encoder input needs none).
"""
import contextlib
import math

import torch

from ._lib import check, lib
from .nn import (LSTM, BiRNN, DeviceLengths, Module, S2SArgumentError, _bytes, _require_cuda_f32, _uniform, dptr,
                 get_context, overlap_param_grads, side_uses, stream_ptr)


def _ctx(t):
    return get_context(t.device.index).handle


class TemporalConvolution(Module):
    """nn.TemporalConvolution(inputFrameSize, outputFrameSize, kW) (dW = 1): weight (out, kW*in), bias (out);
    reset U(+-1/sqrt(kW*in)).  bias=False gives TemporalConvolutionZeroBias (TemporalConvolutionZeroBias.lua)."""

    def __init__(self, inputFrameSize, outputFrameSize, kW, relu=False, bias=True, need_gradInput=True,
                 generator=None):
        super().__init__()
        self.inputFrameSize, self.outputFrameSize, self.kW = inputFrameSize, outputFrameSize, kW
        self.relu, self.need_gradInput = bool(relu), need_gradInput
        stdv = 1.0 / math.sqrt(kW * inputFrameSize)
        self.weight = _uniform((outputFrameSize, kW * inputFrameSize), stdv, generator)
        self.bias = _uniform((outputFrameSize,), stdv, generator) if bias else None
        self.gradWeight = torch.zeros_like(self.weight)
        self.gradBias = torch.zeros_like(self.bias) if bias else None

    def parameters(self):
        ws = [self.weight] + ([self.bias] if self.bias is not None else [])
        gs = [self.gradWeight] + ([self.gradBias] if self.gradBias is not None else [])
        return ws, gs

    def updateOutput(self, input):
        _require_cuda_f32(input, "input")
        self._check_params(input)
        x = input if input.dim() == 3 else input.unsqueeze(0)
        if x.dim() != 3 or x.shape[2] != self.inputFrameSize:
            raise S2SArgumentError("TemporalConvolution: input must be (L, inputFrameSize) or (B, L, inputFrameSize)")
        B, L, _ = x.shape
        y = torch.empty((B, L - self.kW + 1, self.outputFrameSize), device=x.device, dtype=torch.float32)
        check(lib.s2s_tconv_fwd(_ctx(x), stream_ptr(), B, L, self.inputFrameSize, self.outputFrameSize, self.kW,
                                int(self.relu), dptr(x), dptr(self.weight), dptr(self.bias), dptr(y)))
        self.output = y if input.dim() == 3 else y[0]
        return self.output

    def backward(self, input, gradOutput, scale=1.0):
        x = input if input.dim() == 3 else input.unsqueeze(0)
        B, L, _ = x.shape
        go = (gradOutput if gradOutput.dim() == 3 else gradOutput.unsqueeze(0)).contiguous()
        y = self.output if self.output.dim() == 3 else self.output.unsqueeze(0)
        dx = torch.empty_like(x) if self.need_gradInput else None
        scr = _bytes(lib.s2s_tconv_scratch_bytes(B, L, self.inputFrameSize, self.outputFrameSize, self.kW), x.device)
        check(lib.s2s_tconv_bwd(_ctx(x), stream_ptr(), B, L, self.inputFrameSize, self.outputFrameSize, self.kW,
                                int(self.relu), dptr(x), dptr(self.weight), dptr(y), dptr(go), dptr(dx), 0,
                                dptr(self.gradWeight), dptr(self.gradBias), float(scale), dptr(scr), scr.numel()))
        side_uses(x.device, scr)
        self.gradInput = None if dx is None else (dx if input.dim() == 3 else dx[0])
        return self.gradInput


class TemporalMaxPooling(Module):
    """nn.TemporalMaxPooling(kW, dW): floor mode, first maximum wins."""

    def __init__(self, kW, dW=None):
        super().__init__()
        self.kW, self.dW = kW, dW or kW

    def updateOutput(self, input):
        _require_cuda_f32(input, "input")
        self._check_params(input)
        x = input if input.dim() == 3 else input.unsqueeze(0)
        B, L, D = x.shape
        Lo = (L - self.kW) // self.dW + 1
        y = torch.empty((B, Lo, D), device=x.device, dtype=torch.float32)
        self.indices = torch.empty((B, Lo, D), device=x.device, dtype=torch.int32)
        check(lib.s2s_tmaxpool_fwd(_ctx(x), stream_ptr(), B, L, D, self.kW, self.dW, dptr(x), dptr(y),
                                   dptr(self.indices)))
        self.output = y if input.dim() == 3 else y[0]
        return self.output

    def backward(self, input, gradOutput, scale=1.0):
        x = input if input.dim() == 3 else input.unsqueeze(0)
        B, L, D = x.shape
        go = (gradOutput if gradOutput.dim() == 3 else gradOutput.unsqueeze(0)).contiguous()
        dx = torch.empty_like(x)
        check(lib.s2s_tmaxpool_bwd(_ctx(x), stream_ptr(), B, L, D, self.kW, self.dW, dptr(self.indices), dptr(go),
                                   dptr(dx)))
        self.gradInput = dx if input.dim() == 3 else dx[0]
        return self.gradInput


class ReLU(Module):
    """nn.ReLU: y = max(x, 0); dx = dy * 1[x > 0]."""

    def updateOutput(self, input):
        _require_cuda_f32(input, "input")
        self._check_params(input)
        self.output = torch.empty_like(input)
        check(lib.s2s_relu_fwd(_ctx(input), stream_ptr(), input.numel(), dptr(input), dptr(self.output)))
        return self.output

    def backward(self, input, gradOutput, scale=1.0):
        go = gradOutput.contiguous()
        self.gradInput = torch.empty_like(input)
        check(lib.s2s_relu_bwd(_ctx(input), stream_ptr(), input.numel(), dptr(input), dptr(go),
                               dptr(self.gradInput)))
        return self.gradInput


class Linear(TemporalConvolution):
    """nn.Linear(inputSize, outputSize): weight (out, in), bias (out), reset U(+-1/sqrt(in)); rows (N, in) or
    (B, T, in).  Runs as TemporalConvolution(in, out, 1) (one GEMM over the rows, bias in the epilogue)."""

    def __init__(self, inputSize, outputSize, relu=False, generator=None):
        super().__init__(inputSize, outputSize, 1, relu=relu, generator=generator)


class Maxout(Module):
    """nn.Maxout(inputDimension, outputDimension, window) (Maxout.lua:5-19): Linear(in, out*window) ->
    View(out*window, 1) -> TemporalMaxPooling(window, window) -> View(out), on rows (N, in)."""

    def __init__(self, inputDimension, outputDimension, window=4, generator=None):
        super().__init__()
        self.inputDim, self.outputDim, self.window = inputDimension, outputDimension, window
        self.linear = Linear(inputDimension, outputDimension * window, generator=generator)
        self.pool = TemporalMaxPooling(window, window)

    def parameters(self):
        return self.linear.parameters()

    def updateOutput(self, input):
        if input.dim() != 2:
            raise S2SArgumentError("Maxout: rows (N, inputDimension)")
        self._u = self.linear.forward(input)
        N = input.shape[0]
        self.output = self.pool.forward(self._u.reshape(N, -1, 1)).reshape(N, self.outputDim)
        return self.output

    def backward(self, input, gradOutput, scale=1.0):
        N = input.shape[0]
        du = self.pool.backward(self._u.reshape(N, -1, 1), gradOutput.reshape(N, self.outputDim, 1).contiguous())
        self.gradInput = self.linear.backward(input, du.reshape(N, -1), scale)
        return self.gradInput


class LogSoftMax(Module):
    """nn.LogSoftMax over the last dimension."""

    def updateOutput(self, input):
        _require_cuda_f32(input, "input")
        self._check_params(input)
        n = input.shape[-1]
        self.output = torch.empty_like(input)
        check(lib.s2s_logsoftmax_fwd(_ctx(input), stream_ptr(), input.numel() // n, n, dptr(input),
                                     dptr(self.output)))
        return self.output

    def backward(self, input, gradOutput, scale=1.0):
        n = input.shape[-1]
        go = gradOutput.contiguous()
        self.gradInput = torch.empty_like(input)
        check(lib.s2s_logsoftmax_bwd(_ctx(input), stream_ptr(), input.numel() // n, n, dptr(self.output), dptr(go),
                                     dptr(self.gradInput)))
        return self.gradInput


class SpatialConvolutionMM(Module):
    """nn.SpatialConvolutionMM(nInputPlane, nOutputPlane, kW, kH) (stride 1, no padding): weight
    (out, in*kH*kW), bias (out); reset U(+-1/sqrt(kW*kH*in)).  Input (B, C, H, W) or (C, H, W)."""

    def __init__(self, nInputPlane, nOutputPlane, kW, kH=None, relu=False, need_gradInput=True, generator=None):
        super().__init__()
        self.nInputPlane, self.nOutputPlane, self.kW, self.kH = nInputPlane, nOutputPlane, kW, kH or kW
        self.relu, self.need_gradInput = bool(relu), need_gradInput
        stdv = 1.0 / math.sqrt(self.kW * self.kH * nInputPlane)
        self.weight = _uniform((nOutputPlane, nInputPlane * self.kH * self.kW), stdv, generator)
        self.bias = _uniform((nOutputPlane,), stdv, generator)
        self.gradWeight = torch.zeros_like(self.weight)
        self.gradBias = torch.zeros_like(self.bias)

    def parameters(self):
        return [self.weight, self.bias], [self.gradWeight, self.gradBias]

    def _dims(self, x):
        if x.dim() != 4 or x.shape[1] != self.nInputPlane:
            raise S2SArgumentError("SpatialConvolutionMM: input must be (C, H, W) or (B, C, H, W) with C = nInputPlane")
        return x.shape

    def updateOutput(self, input):
        _require_cuda_f32(input, "input")
        self._check_params(input)
        x = input if input.dim() == 4 else input.unsqueeze(0)
        B, C, H, W = self._dims(x)
        y = torch.empty((B, self.nOutputPlane, H - self.kH + 1, W - self.kW + 1), device=x.device,
                        dtype=torch.float32)
        scr = _bytes(lib.s2s_sconv_scratch_bytes(B, C, H, W, self.nOutputPlane, self.kH, self.kW), x.device)
        self._scr = (scr, x.data_ptr(), x.shape)  # the im2col panel, reused by the backward on the same input
        check(lib.s2s_sconv_fwd(_ctx(x), stream_ptr(), B, C, H, W, self.nOutputPlane, self.kH, self.kW,
                                int(self.relu), dptr(x), dptr(self.weight), dptr(self.bias), dptr(y), dptr(scr),
                                scr.numel()))
        self.output = y if input.dim() == 4 else y[0]
        return self.output

    def backward(self, input, gradOutput, scale=1.0):
        x = input if input.dim() == 4 else input.unsqueeze(0)
        B, C, H, W = self._dims(x)
        go = (gradOutput if gradOutput.dim() == 4 else gradOutput.unsqueeze(0)).contiguous()
        y = self.output if self.output.dim() == 4 else self.output.unsqueeze(0)
        dx = torch.empty_like(x) if self.need_gradInput else None
        saved = getattr(self, "_scr", None)
        reuse = saved is not None and saved[1] == x.data_ptr() and saved[2] == x.shape
        scr = saved[0] if reuse else _bytes(lib.s2s_sconv_scratch_bytes(B, C, H, W, self.nOutputPlane, self.kH,
                                                                         self.kW), x.device)
        check(lib.s2s_sconv_bwd(_ctx(x), stream_ptr(), B, C, H, W, self.nOutputPlane, self.kH, self.kW,
                                int(self.relu), dptr(x), dptr(self.weight), dptr(y), dptr(go), dptr(dx), 0,
                                dptr(self.gradWeight), dptr(self.gradBias), float(scale), dptr(scr), scr.numel(),
                                int(reuse)))
        self._scr = None
        self.gradInput = None if dx is None else (dx if input.dim() == 4 else dx[0])
        return self.gradInput


class SpatialMaxPooling(Module):
    """nn.SpatialMaxPooling(kW, kH, dW, dH) (floor mode, first maximum wins)."""

    def __init__(self, kW, kH, dW=None, dH=None):
        super().__init__()
        self.kW, self.kH, self.dW, self.dH = kW, kH, dW or kW, dH or kH

    def updateOutput(self, input):
        _require_cuda_f32(input, "input")
        self._check_params(input)
        x = input if input.dim() == 4 else input.unsqueeze(0)
        B, C, H, W = x.shape
        Ho, Wo = (H - self.kH) // self.dH + 1, (W - self.kW) // self.dW + 1
        y = torch.empty((B, C, Ho, Wo), device=x.device, dtype=torch.float32)
        self.indices = torch.empty((B, C, Ho, Wo), device=x.device, dtype=torch.int32)
        check(lib.s2s_smaxpool_fwd(_ctx(x), stream_ptr(), B, C, H, W, self.kW, self.kH, self.dW, self.dH, dptr(x),
                                   dptr(y), dptr(self.indices)))
        self.output = y if input.dim() == 4 else y[0]
        return self.output

    def backward(self, input, gradOutput, scale=1.0):
        x = input if input.dim() == 4 else input.unsqueeze(0)
        B, C, H, W = x.shape
        go = (gradOutput if gradOutput.dim() == 4 else gradOutput.unsqueeze(0)).contiguous()
        dx = torch.empty_like(x)
        check(lib.s2s_smaxpool_bwd(_ctx(x), stream_ptr(), B, C, H, W, self.kW, self.kH, self.dW, self.dH,
                                   dptr(self.indices), dptr(go), dptr(dx)))
        self.gradInput = dx if input.dim() == 4 else dx[0]
        return self.gradInput


class Transpose2(Module):
    """nn.Transpose2({1,2},3) (Transpose2.lua): (nFeat, L, H) -> (L, nFeat, H), batched (B, nFeat, L, H) ->
    (B, L, nFeat, H).  Only this permutation (the one model_vgg.lua:41 uses) runs on this path."""

    def __init__(self, *perms):
        super().__init__()
        if perms not in (((1, 2), 3), ([1, 2], 3)):
            raise S2SArgumentError("Transpose2: only ({1,2}, 3) is implemented")

    def updateOutput(self, input):
        _require_cuda_f32(input, "input")
        self._check_params(input)
        if input.dim() not in (3, 4):
            raise S2SArgumentError("inconsistent tensor size")  # Transpose2.lua:29
        x = input if input.dim() == 4 else input.unsqueeze(0)
        B, D1, D2, D3 = x.shape
        y = torch.empty((B, D2, D1, D3), device=x.device, dtype=torch.float32)
        check(lib.s2s_swap12(_ctx(x), stream_ptr(), B, D1, D2, D3, dptr(x), dptr(y)))
        self.output = y if input.dim() == 4 else y[0]
        return self.output

    def backward(self, input, gradOutput, scale=1.0):
        x = input if input.dim() == 4 else input.unsqueeze(0)
        B, D1, D2, D3 = x.shape
        go = (gradOutput if gradOutput.dim() == 4 else gradOutput.unsqueeze(0)).contiguous()
        dx = torch.empty_like(x)
        check(lib.s2s_swap12(_ctx(x), stream_ptr(), B, D2, D1, D3, dptr(go), dptr(dx)))
        self.gradInput = dx if input.dim() == 4 else dx[0]
        return self.gradInput


class View(Module):
    """nn.View(-1, n):setNumInputDims(3) on a batch: (B, L, C, H) -> (B, L, C*H) (a free reshape)."""

    def updateOutput(self, input):
        self.output = input.reshape(input.shape[0], input.shape[1], -1)
        return self.output

    def backward(self, input, gradOutput, scale=1.0):
        self.gradInput = gradOutput.reshape(input.shape)
        return self.gradInput


class Sequential(Module):
    """nn.Sequential: forward in order, backward in reverse (each module's backward = updateGradInput +
    accGradParameters)."""

    def __init__(self, *modules):
        super().__init__()
        self.modules = list(modules)

    def add(self, m):
        self.modules.append(m)
        return self

    def parameters(self):
        ws, gs = [], []
        for m in self.modules:
            w, g = m.parameters()
            ws += w
            gs += g
        return ws, gs

    def updateOutput(self, input):
        self._inputs = []
        h = input
        for m in self.modules:
            self._inputs.append(h)
            h = m.forward(h)
        self.output = h
        return h

    def backward(self, input, gradOutput, scale=1.0):
        d = gradOutput
        for m, x in zip(reversed(self.modules), reversed(self._inputs)):
            d = m.backward(x, d, scale)
        self.gradInput = d
        return d


class ConvBiLSTMEncoder(Module):
    """timit/timit.lua:108-125: convlayer = 3 x [TemporalConvolution(D, hidden, kW) -> ReLU ->
    TemporalMaxPooling(2, 2)], applied once and read by both RNN(LSTM(hidden, out, peepholes=nil))
    directions (the reference calls the same module on the same input twice, :123-124, so the
    forward is one conv stack and its weight gradients sum both directions' contributions), then
    JoinTable(2,2).  x (B, L, D) -> (B, L', 2*out), L' = three times (L - kW + 1) // 2."""

    def __init__(self, inputFrameSize, hiddenFrameSize=256, outputFrameSize=128, kW=3, generator=None):
        super().__init__()
        convs = []
        for l in range(3):
            convs += [TemporalConvolution(inputFrameSize if l == 0 else hiddenFrameSize, hiddenFrameSize, kW, relu=True,
                                          need_gradInput=l > 0, generator=generator),
                      TemporalMaxPooling(2, 2)]
        self.convlayer = Sequential(*convs)
        self.rnn = BiRNN(LSTM(hiddenFrameSize, outputFrameSize, False, generator),
                         LSTM(hiddenFrameSize, outputFrameSize, False, generator))

    def parameters(self):
        w1, g1 = self.convlayer.parameters()
        w2, g2 = self.rnn.parameters()
        return w1 + w2, g1 + g2

    def out_lengths(self, Ls):
        """Annotation frames L' per utterance of Ls raw frames: L -> (L - kW + 1) // 2 once per conv + pool stage.
        An utterance that keeps no frame raises S2SArgumentError (kW = 3: at least 22 frames)."""
        kW = self.convlayer.modules[0].kW
        need = 1
        for _ in range(3):
            need = 2 * need + kW - 1
        out = []
        for L in Ls:
            L = int(L)
            if L < need:
                raise S2SArgumentError(f"ConvBiLSTMEncoder: an utterance of {L} frames keeps no annotation frame "
                                       f"(the minimum is {need})")
            for _ in range(3):
                L = (L - kW + 1) // 2
            out.append(L)
        return out

    def updateOutput(self, input):
        self._c = self.convlayer.forward(input)
        self.output = self.rnn.forward(self._c)
        return self.output

    def backward(self, input, gradOutput, scale=1.0):
        dc = self.rnn.backward(self._c, gradOutput, scale)  # sum of both directions' dx
        self.gradInput = self.convlayer.backward(input, dc, scale)
        return self.gradInput


class VGGEncoder(Module):
    """librispeech/model_vgg.lua:23-51 on x (B, 3, L, F) (H = time, W = frequency) -> (B, (L-8)//2, out):
    SpatialConvolutionMM(3,64,3,3)+ReLU, (64,64)+ReLU, SpatialMaxPooling(2,1,2,1), (64,128)+ReLU,
    (128,128)+ReLU, SpatialMaxPooling(2,2,2,2), Transpose2({1,2},3), View(-1, 128*H'), then
    TemporalConvolution(128*H', hidden, 1), (hidden, hidden, 1) x 2, (hidden, out, 1), each + ReLU."""

    def __init__(self, inputFrameSize=40, outputFrameSize=512, hidden=2048, generator=None):
        super().__init__()
        Hf = ((inputFrameSize - 4) // 2 - 4) // 2
        if Hf < 1:
            raise S2SArgumentError("VGGEncoder: inputFrameSize too small for the conv stack")
        g = generator
        self.seq = Sequential(
            SpatialConvolutionMM(3, 64, 3, 3, relu=True, need_gradInput=False, generator=g),
            SpatialConvolutionMM(64, 64, 3, 3, relu=True, generator=g),
            SpatialMaxPooling(2, 1, 2, 1),
            SpatialConvolutionMM(64, 128, 3, 3, relu=True, generator=g),
            SpatialConvolutionMM(128, 128, 3, 3, relu=True, generator=g),
            SpatialMaxPooling(2, 2, 2, 2),
            Transpose2((1, 2), 3),
            View(),
            TemporalConvolution(128 * Hf, hidden, 1, relu=True, generator=g),
            TemporalConvolution(hidden, hidden, 1, relu=True, generator=g),
            TemporalConvolution(hidden, hidden, 1, relu=True, generator=g),
            TemporalConvolution(hidden, outputFrameSize, 1, relu=True, generator=g))

    def parameters(self):
        return self.seq.parameters()

    def out_lengths(self, Ls):
        """Annotation frames L' = (L - 8) // 2 per utterance of Ls raw frames (four 3x3 convolutions, the second
        pooling halves time); an utterance under 10 frames keeps none and raises S2SArgumentError."""
        for L in Ls:
            if int(L) < 10:
                raise S2SArgumentError(f"VGGEncoder: an utterance of {int(L)} frames keeps no annotation frame "
                                       "(the minimum is 10)")
        return [(int(L) - 8) // 2 for L in Ls]

    def updateOutput(self, input):
        self.output = self.seq.forward(input)
        return self.output

    def backward(self, input, gradOutput, scale=1.0):
        self.gradInput = self.seq.backward(input, gradOutput, scale)
        return self.gradInput


class GraphStep:
    """graph_step() for the host-side models (VGGAttentionModel, ConvBiLSTMAttentionModel): their step is a
    sequence of module calls from Python (front-end Sequential, decoder, decoder_mlp, loss seed and every
    backward), hundreds of launches -- the per-step decoder kernels of the conv + BiLSTM model alone launch a
    handful per decoder step -- replayed from one captured HIP graph."""

    def graph_step(self, x, labels, scale=None, normalizeNLL=False, frame_lengths=None, label_lengths=None):
        """zeroGradParameters() + step() replayed from a captured HIP graph: every launch of the host-side
        step (front-end, decoder, decoder_mlp, loss seed and every backward) becomes one graph launch.  The
        capture is keyed by the input / label buffers (pointers and shapes): refill x and labels in place to
        train on new data.  The first call of a key runs one eager step
        (which sizes every lazily grown buffer, so the capture allocates only from its graph pool), then
        captures and replays; the returned (nll, logp) are the graph's own buffers, rewritten by every
        replay.  grads = this step's gradient (the graph zeroes them first).
        frame_lengths / label_lengths: DeviceLengths of a padded batch; their device pointers are part of the key
        and the kernels read the values at replay time, so fill_() them in place with the next batch's lengths
        (PackedUtterances.batch(out=...) does) and replay.  A new padded shape is a new capture."""
        for ln in (frame_lengths, label_lengths):
            if ln is not None and not isinstance(ln, DeviceLengths):
                raise S2SArgumentError("graph_step: lengths must be DeviceLengths (a captured step reads them on the "
                                       "device at replay time)")
        key = (x.data_ptr(), tuple(x.shape), labels.data_ptr(), tuple(labels.shape), scale, normalizeNLL)
        if frame_lengths is not None or label_lengths is not None:
            key += tuple(None if ln is None else ln.tensor.data_ptr() for ln in (frame_lengths, label_lengths))
        lens = {} if frame_lengths is None and label_lengths is None else dict(frame_lengths=frame_lengths,
                                                                              label_lengths=label_lengths)
        graphs = self.__dict__.setdefault("_graphs", {})
        g = graphs.get(key)
        if g is None:
            # the eager step runs on the capture stream: the library's lazily grown per-stream buffers (the big
            # bf16 GEMMs' staging copies) are sized for THAT stream before the capture, which cannot allocate them
            # one capture stream per model: the library keeps a few per-stream staging buffers, so a
            # fresh stream per key would use them up with shapes (ragged batches) and leave dead streams' buffers
            cur = torch.cuda.current_stream(x.device)
            side = self.__dict__.get("_capture_stream")
            if side is None or side.device != x.device:
                side = self.__dict__["_capture_stream"] = torch.cuda.Stream(x.device)
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                self.zeroGradParameters()
                self.step(x, labels, scale, normalizeNLL, **lens)
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
                self.zeroGradParameters()
                out = self.step(x, labels, scale, normalizeNLL, **lens)
            cur.wait_stream(side)
            graphs[key] = g = (graph, out)
        g[0].replay()
        return g[1]



class RaggedModel:
    """step / forward / step_ragged / BeamSearch / Evaluate of the host-side models on padded batches of
    variable-length utterances: the reference runs them one utterance at a time (timit/timit.lua:239-295 and
    :368-417, librispeech/train.lua:82-261).  The front-end runs on the padded batch unmasked (no padding in its
    convolutions and poolings: output frame j < L'_b reads only input frames < L_b); every reader of its output is
    masked by L' = encoder.out_lengths(L) -- the BiLSTM (lengths), the decoder (frame_lengths) -- and hands back
    exact zeros on the padding, so no gradient reaches a parameter from there."""

    def _lengths(self, x, labels, frame_lengths, label_lengths):
        """(L' DeviceLengths, label DeviceLengths) of a padded batch, either None when not given.  Lists are checked
        and uploaded once here; DeviceLengths are used as they are (their derived L' follows every fill_)."""
        lp = tl = None
        if frame_lengths is None and label_lengths is None:
            return lp, tl
        if x.dim() != self._time_axis + 2 or labels.dim() != 2 or labels.shape[0] != x.shape[0]:
            raise S2SArgumentError(f"{type(self).__name__}: with lengths x must have {self._time_axis + 2} dimensions "
                                   "and labels be (B, T)")
        B, L, T = x.shape[0], x.shape[self._time_axis], labels.shape[1]
        if frame_lengths is not None:
            fl = frame_lengths
            if not isinstance(fl, DeviceLengths):
                fl = DeviceLengths(frame_lengths, L, x.device)
            fl.ptr(B, L)
            Lp = self.encoder.out_lengths([L])[0]
            lp = fl.derive(type(self.encoder).__name__, self.encoder.out_lengths, Lp)
        if label_lengths is not None:
            tl = label_lengths
            if not isinstance(tl, DeviceLengths):
                tl = DeviceLengths(label_lengths, T, x.device)
            tl.ptr(B, T)
        return lp, tl

    def _run(self, x, labels, scale, normalizeNLL, frame_lengths, label_lengths, backward):
        from .nn import nll_seed, precision
        B = x.shape[0]
        scale = (1.0 / B if B > 1 else 1.0) if scale is None else scale
        lp, tl = self._lengths(x, labels, frame_lengths, label_lengths)
        rnn, dec = getattr(self.encoder, "rnn", None), self.decoder
        was = (rnn.lengths if rnn is not None else None, dec.frame_lengths, dec.label_lengths)
        if rnn is not None:
            rnn.lengths = lp
        dec.frame_lengths, dec.label_lengths = lp, tl
        try:
            with precision(self.precision, x.device.index):
                h = self.encoder.forward(x)
                lab = labels.to(torch.int32).contiguous()
                logp = dec.forward([h, lab])
                nll, dlogp = nll_seed(logp, lab, normalizeNLL, tl)
                if backward:
                    # each module's parameter gradients beside the next module's backward (bitwise the serial sums)
                    with overlap_param_grads(x.device.index) if self.overlap else contextlib.nullcontext():
                        dh = dec.backward([h, lab], dlogp, scale)[0]
                        self.encoder.backward(x, dh, scale)
        finally:
            if rnn is not None:
                rnn.lengths = was[0]
            dec.frame_lengths, dec.label_lengths = was[1], was[2]
        return nll, logp

    def step(self, x, labels, scale=None, normalizeNLL=False, frame_lengths=None, label_lengths=None):
        """One training step on a batch x (VGG: (B, 3, L, F); conv + BiLSTM: (B, L, D)), labels (B, T) 0-based:
        forward, nll, backward with gradients accumulated at scale (default 1/B).  Returns (nll (B,), logp
        (B, T, O)).  frame_lengths / label_lengths (B,) (lists, tensors or DeviceLengths): raw frames and labels
        per utterance of a padded batch -- the step then equals the reference's loop over the unpadded utterances;
        logp rows past T_b are padding.  Without them: a batch of equal-length utterances, as before."""
        return self._run(x, labels, scale, normalizeNLL, frame_lengths, label_lengths, True)

    def forward(self, x, labels, scale=None, normalizeNLL=False, frame_lengths=None, label_lengths=None):
        """The validation pass (timit/timit.lua:368-417): the step's forward and nll in evaluate() mode with no
        backward -- no gradient is read or written.  Returns (nll, logp), bitwise a step's on the same inputs;
        encoder.output and the decoder's accessors are valid afterwards."""
        was_train, self.train = self.train, False
        try:
            return self._run(x, labels, scale, normalizeNLL, frame_lengths, label_lengths, False)
        finally:
            self.train = was_train

    @staticmethod
    def _round_up(n, m):
        return n if not m else (n + m - 1) // m * m

    def step_ragged(self, xs, labels, max_batch=None, normalizeNLL=False, graph=False, length_multiple=None):
        """The reference's minibatch over variable-length utterances (one forward / backward per utterance,
        gradients summed, then / N) as padded, length-masked steps: sorted by length, cut into batches of at most
        max_batch, each assembled on the device (PackedUtterances) and run with lengths, accumulating at scale
        1/N.  xs: the utterances ((L_i, D) or (3, L_i, F)) with labels[i] (T_i,), or a PackedUtterances (labels
        None) to pack a corpus once.  graph=True replays each padded shape's step from a captured graph (the
        batch buffers and DeviceLengths are kept per shape and refilled in place); length_multiple = m rounds Lmax
        and Tmax up to multiples of m so that captures get reused -- further padding changes no result.
        Returns nll (N,) in input order and the per-utterance logp list ((T_i, O) each).  Gradients are zeroed
        first."""
        from .data import PackedUtterances
        pk = xs if isinstance(xs, PackedUtterances) else PackedUtterances(xs, labels)
        N = len(pk)
        self.encoder.out_lengths(pk.Ls)  # refuses an utterance below the minimum before anything runs
        scale = 1.0 / N if N > 1 else 1.0
        order = sorted(range(N), key=lambda i: (pk.Ls[i], pk.Ts[i]))
        nb = int(max_batch or N)
        dev = None
        nll, logps = None, [None] * N
        bufs = self.__dict__.setdefault("_ragged_bufs", {})
        self.zeroGradParameters()
        for c0 in range(0, N, nb):
            idx = order[c0:c0 + nb]
            Lmax = self._round_up(max(pk.Ls[i] for i in idx), length_multiple)
            Tmax = self._round_up(max(pk.Ts[i] for i in idx), length_multiple)
            if graph:
                key = (len(idx), Lmax, Tmax)
                bt = bufs[key] = pk.batch(idx, Lmax, Tmax, out=bufs.get(key))
                x, y, fl, tl, _, Ts = bt
                acc = self.__dict__.setdefault("_ragged_acc", [torch.zeros_like(g) for g in self.parameters()[1]])
                if c0 == 0:
                    torch._foreach_zero_(acc)
                n, lp = self.graph_step(x, y, scale, normalizeNLL, fl, tl)  # (zeroes the gradients it writes)
                torch._foreach_add_(acc, self.parameters()[1])
            else:
                x, y, fl, tl, _, Ts = pk.batch(idx, Lmax, Tmax)
                n, lp = self.step(x, y, scale, normalizeNLL, fl, tl)
            if nll is None:
                dev = x.device
                nll = torch.empty(N, device=dev, dtype=torch.float32)
            nll[torch.tensor(idx, device=dev)] = n
            for j, i in enumerate(idx):
                logps[i] = lp[j, :Ts[j]].clone()
        if graph:
            for g, a in zip(self.parameters()[1], acc):
                g.copy_(a)
        return nll, logps

    def BeamSearch(self, eos, K=5, maxseqlength=None, frame_lengths=None, maxseqlengths=None):
        """decoder:BeamSearch(encoder.output, eos, K, maxseqlen) on the annotations of the last step / forward.
        frame_lengths (B,): annotation frames L'_b of a padded batch (content attention, or a hybrid decoder with
        decoder.share_hybrid_search on; otherwise the hybrid decoder refuses them and Evaluate searches equal-L'
        groups instead).  Returns (tokens (B, maxseqlength + 1) padded
        with -1, lengths (B), scores (B))."""
        h = self.encoder.output
        if h is None:
            raise S2SArgumentError("BeamSearch: run step() or forward() first")
        return self.decoder.BeamSearch(h if h.dim() == 3 else h[None], eos, K, maxseqlength,
                                       frame_lengths=frame_lengths, maxseqlengths=maxseqlengths)

    def Evaluate(self, xs, ys, K=5, max_batch=32, eos=None, token_map=None, maxlen_factor=None):
        """Evaluate(data) (timit/timit.lua:368-417; librispeech/train.lua:222-261) over utterances xs[i] with
        labels ys[i] (T_i,) 0-based (or a PackedUtterances and ys = None), in evaluate() mode: sorted by length,
        cut into padded batches of at most max_batch, each run through forward() with lengths, then the beam
        search (_search) with each utterance's own limit maxlen_factor * L_b raw frames (default: the model's
        reference trainer's), then the edit distance on the device.  eos = the last label, the same for every
        utterance (ValueError otherwise); token_map (O,) is applied to prediction and target before the distance.
        Returns (accuracy = sum numCorrect / sum T_b, NLL = sum_b nll_b / N unnormalised, PER or CER = mean_b
        dist_b / T_b, predlist: the unmapped predictions, int64 CPU tensors), all in input order.
        self.eval_detail keeps the per-utterance nll, numCorrect, distances and beam scores; self.eval_groups the
        searches that ran, as (L' or None, [positions in their batch])."""
        from .data import PackedUtterances
        from .nn import edit_distance
        pk = xs if isinstance(xs, PackedUtterances) else None
        N = len(xs)
        if N == 0 or (pk is None and len(ys) != N):
            raise ValueError("Evaluate needs one label sequence per utterance")
        if pk is None:
            labs = [torch.as_tensor(y).to(torch.int64).reshape(-1).cpu() for y in ys]
        else:
            labs = [y.to(torch.int64).cpu() for y in (pk._ys or pk.y.cpu().split(pk.Ts))]
        if any(y.numel() == 0 for y in labs):
            raise ValueError("Evaluate: empty label sequence")
        lasts = {int(y[-1]) for y in labs}
        if eos is not None:
            lasts.add(int(eos))
        if len(lasts) != 1:
            raise ValueError(f"Evaluate: eos (the last label) differs between utterances: {sorted(lasts)}")
        eos = lasts.pop()
        if pk is None:
            pk = PackedUtterances(xs, labs)
        factor = int(self.maxlen_factor if maxlen_factor is None else maxlen_factor)
        if factor < 1:
            raise ValueError("Evaluate: maxlen_factor must be at least 1")
        self.encoder.out_lengths(pk.Ls)
        O = self.decoder.outputDepth
        if token_map is not None and torch.as_tensor(token_map).numel() != O:
            raise ValueError("token_map must have outputDepth entries")
        nll, correct, dist, score, preds = [0.0] * N, [0] * N, [0] * N, [0.0] * N, [None] * N
        order = sorted(range(N), key=lambda i: (pk.Ls[i], pk.Ts[i]))
        self.eval_groups = []
        tmap = None
        for c0 in range(0, N, int(max_batch)):
            idx = order[c0:c0 + int(max_batch)]
            x, y, fl, tl, Ls, Ts = pk.batch(idx)
            dev = x.device
            if token_map is not None and tmap is None:
                tmap = torch.as_tensor(token_map).to(torch.int32).reshape(-1).to(dev)
            n, logp = self.forward(x, y, None, False, fl, tl)
            live = torch.arange(y.shape[1], device=dev)[None, :] < tl.tensor[:, None]
            ok = ((logp.argmax(-1).to(torch.int32) == y) & live).sum(1)
            out, olen, osc = self._search(self.encoder.output, self.encoder.out_lengths(Ls), [factor * L for L in Ls],
                                          eos, K)
            pm, tm = out, y
            if tmap is not None:
                pm = torch.where(out >= 0, tmap[out.clamp(min=0).long()], out)
                tm = tmap[y.long()]
            dd = edit_distance(pm, olen, tm, tl.tensor)
            n_c, ok_c, dd_c, out_c, olen_c, osc_c = (t.cpu() for t in (n, ok, dd, out, olen, osc))
            for j, i in enumerate(idx):
                nll[i], correct[i], dist[i], score[i] = float(n_c[j]), int(ok_c[j]), int(dd_c[j]), float(osc_c[j])
                preds[i] = out_c[j, :int(olen_c[j])].to(torch.int64).clone()
        Tn = [y.numel() for y in labs]
        self.eval_detail = {"nll": nll, "numCorrect": correct, "dist": dist, "score": score, "T": Tn}
        accuracy = sum(correct) / sum(Tn)
        per = [dist[i] / Tn[i] for i in range(N)]
        return accuracy, sum(nll) / N, sum(per) / N, preds


class VGGAttentionModel(RaggedModel, GraphStep, Module):
    """librispeech/model_vgg.lua:loadmodel(opt) end to end: VGGEncoder -> nn.Attention(GRU(S, S),
    decoder_mlp = Maxout(S+A, M, 7) -> Linear(M, M) -> Maxout(M, M, 7) -> Linear(M, O) -> LogSoftMax
    (:71-77), scoreDepth, hybrid (off by default), S, A, O, monoAlignPenalty = true, penalty) with the
    loss seed of librispeech/train.lua (nll = -sum labelmask * logp, dlogp = -labelmask, grads / B).
    The decoder_mlp runs outside the decoder launches on the saved [s_t; c_t] rows (external_mlp)."""

    def __init__(self, inputFrameSize=40, outputFrameSize=512, hidden=2048, scoreDepth=512, stateDepth=256,
                 outputDepth=62, mlpDepth=64, penalty=0.0, generator=None, precision="fp32"):
        from .nn import GRU, Attention
        super().__init__()
        # "bf16": every hoisted GEMM of the step (the VGG convolutions and 1x1 layers, Vh, decoder folds, the
        # decoder_mlp Linears, all weight gradients) on bf16 MFMA with fp32 accumulation (BASELINE config 5)
        self.precision = precision
        self.overlap = True  # parameter gradients on the side stream during the backward (overlap_param_grads)
        g = generator
        S, A, M, O = stateDepth, outputFrameSize, mlpDepth, outputDepth
        self.encoder = VGGEncoder(inputFrameSize, outputFrameSize, hidden, generator=g)
        mlp = Sequential(Maxout(S + A, M, 7, generator=g), Linear(M, M, generator=g), Maxout(M, M, 7, generator=g),
                         Linear(M, O, generator=g), LogSoftMax())
        self.decoder = Attention(GRU(S, S, generator=g), mlp, scoreDepth, 10, 0, S, A, O, True, penalty, generator=g)

    def parameters(self):
        w1, g1 = self.encoder.parameters()
        w2, g2 = self.decoder.parameters()
        return w1 + w2, g1 + g2

    _time_axis = 2      # x (B, 3, L, F); one utterance (3, L, F)
    maxlen_factor = 2   # librispeech/train.lua:251: the search runs to twice the utterance's input frames

    def _search(self, h, Lp, limits, eos, K):
        """One ragged search over the padded annotations (frames >= L'_b take no part)."""
        out, olen, osc = self.decoder.BeamSearch(h, eos, K, max(limits), frame_lengths=Lp, maxseqlengths=limits)
        self.eval_groups.append((None, list(range(h.shape[0]))))
        return out, olen, osc


class ConvBiLSTMAttentionModel(RaggedModel, GraphStep, Module):
    """The conv + BiLSTM model timit/timit.lua builds when no model file is given (:106-145), end to end:
    ConvBiLSTMEncoder (3 x conv(k=3, 256) + ReLU + TemporalMaxPooling(2, 2), BiLSTM 2 x 128) ->
    nn.Attention(decoder_recurrent = LSTM(400, 400), decoder_mlp = Linear(400 + 256, 2*O) -> ReLU ->
    Linear(2*O, O) -> LogSoftMax, scoreDepth 150, hybrid attention kW = 5 / 16 maps, monoAlignPenalty
    true, opt.penalty), with the trainer's loss seed (timit/timit.lua:262-295)."""

    def __init__(self, inputFrameSize=123, numPhonemes=62, hiddenFrameSize=256, outputFrameSize=128,
                 stateDepth=400, scoreDepth=150, hybridAttendFilterSize=5, hybridAttendFeatureMaps=16, penalty=0.0,
                 generator=None, precision="fp32"):
        from .nn import Attention
        super().__init__()
        self.precision = precision  # "fp32" | "bf16" | "bf16-all" (s2s_amd.precision) for the step's GEMMs
        self.overlap = True  # parameter gradients on the side stream during the backward (overlap_param_grads)
        g = generator
        S, A, O = stateDepth, 2 * outputFrameSize, numPhonemes
        self.encoder = ConvBiLSTMEncoder(inputFrameSize, hiddenFrameSize, outputFrameSize, 3, generator=g)
        mlp = Sequential(Linear(S + A, 2 * O, generator=g), ReLU(), Linear(2 * O, O, generator=g), LogSoftMax())
        self.decoder = Attention(LSTM(S, S, False, g), mlp, scoreDepth, hybridAttendFilterSize,
                                 hybridAttendFeatureMaps, S, A, O, True, penalty, generator=g)

    def parameters(self):
        w1, g1 = self.encoder.parameters()
        w2, g2 = self.decoder.parameters()
        return w1 + w2, g1 + g2

    _time_axis = 1      # x (B, L, D); one utterance (L, D)
    maxlen_factor = 1   # timit/timit.lua:400: the search runs to the utterance's own frame count

    def _search(self, h, Lp, limits, eos, K):
        """By default hybrid attention takes no frame lengths in the search, and three halvings leave few distinct
        L': the annotation rows are gathered by equal L' into unpadded (B_g, L', A) groups, one search per group.
        With decoder.share_hybrid_search the padded batch is searched in one ragged call, as the VGG model's is."""
        if self.decoder.share_hybrid_search:
            return VGGAttentionModel._search(self, h, Lp, limits, eos, K)
        B, dev = h.shape[0], h.device
        maxlen = max(limits)
        out = torch.full((B, maxlen + 1), -1, dtype=torch.int32, device=dev)
        olen = torch.empty(B, dtype=torch.int32, device=dev)
        osc = torch.empty(B, dtype=torch.float32, device=dev)
        for lp in sorted(set(Lp)):
            rows = [j for j in range(B) if Lp[j] == lp]
            sel = torch.tensor(rows, device=dev)
            lim = [limits[j] for j in rows]
            o, n, sc = self.decoder.BeamSearch(h[sel, :lp].contiguous(), eos, K, max(lim), maxseqlengths=lim)
            out[sel, :o.shape[1]] = o
            olen[sel], osc[sel] = n, sc
            self.eval_groups.append((lp, rows))
        return out, olen, osc

"""ResNet-34 / ResNet-50 classifiers over the HIP kernels of csrc/classify.hip and csrc/conv.hip, inference only.

Restates torchvision's published ``ResNet`` (v1.5: in ``Bottleneck`` the stride sits on the 3x3) with torchvision's ``state_dict`` keys --
the models DDPM/classifier_evaluation.py:135-143 (``resnet34`` with a 10-way ``fc``) and SD/eval-scripts/imageclassify.py:41-44 (``resnet50``)
load.  torchvision is not part of this project's environment, so parity at that boundary is unpinned.

BatchNorm is eval-mode only and is folded into the convolution before it at load, in fp64 on the host (``fold_bn``): w' = w * s,
b' = beta - mean * s, s = gamma / sqrt(var + 1e-5).  w' goes to an fp32 arena and its bf16 shadow (the GEMM operands), b' stays fp32 and is
added in the convolution's epilogue together with the fp32 residual.  Activations are NHWC rows: fp32 where they are a residual, bf16 where
they feed a product, in a few workspaces reused across calls, on the current stream.

The stem is a patch matrix (sfron_image_u8_patches7 / sfron_nchw_patches7) times the [64][k_pad] weights on the plain GEMM; every other
convolution is sfron_conv_fwd (3x3 and 1x1, stride 1 and 2); the head is sfron_pool_fc in fp32.

Chunk invariant (forward_net.py, as vae.py): the library refuses an operand of 2 GiB or more, so a batch runs in chunks of samples whose
largest operand stays under ``max_chunk_bytes``; every launch asserts its operands are below 2 GiB.
"""
import ctypes
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from ._lib import check, lib as _L, ptr, stream_ptr
from .forward_net import ForwardNet, guard

BN_EPS = 1e-5
STEM_K = 147                 # 7 * 7 * 3 live columns of the stem's patch matrix
STEM_K_PAD = 152             # ... padded to a multiple of 8


class BasicBlock:
    """Marker of torchvision's BasicBlock (3x3, 3x3): ResNet-18 / 34."""
    expansion = 1


class Bottleneck:
    """Marker of torchvision's Bottleneck (1x1, 3x3 with the stride, 1x1): ResNet-50 and up."""
    expansion = 4


def fold_bn(w, gamma, beta, mean, var, eps=BN_EPS):
    """(w', b') in fp64: conv(x, w') + b' == BatchNorm(conv(x, w)) in eval mode."""
    w, gamma, beta, mean, var = (torch.as_tensor(t).detach().to("cpu", torch.float64) for t in (w, gamma, beta, mean, var))
    s = gamma / torch.sqrt(var + eps)
    return w * s.view(-1, 1, 1, 1), beta - mean * s


def resnet_plan(block, layers, num_classes=1000):
    """(specs, convs, blocks): ``specs`` {state_dict key: shape} in torchvision's order; ``convs`` [(conv key, bn key, c_in, c_out, k, stride,
    pad)] with the stem first; ``blocks`` [(prefix, [conv indices], downsample conv index or None)] in execution order."""
    specs, convs, blocks = OrderedDict(), [], []

    def conv_bn(conv, bn, cin, cout, k, stride, pad):
        specs[conv + ".weight"] = (cout, cin, k, k)
        for n in ("weight", "bias", "running_mean", "running_var"):
            specs[f"{bn}.{n}"] = (cout,)
        specs[bn + ".num_batches_tracked"] = ()
        convs.append((conv, bn, cin, cout, k, stride, pad))
        return len(convs) - 1

    conv_bn("conv1", "bn1", 3, 64, 7, 2, 3)
    inplanes = 64
    for li, n in enumerate(layers):
        planes = 64 * 2 ** li
        for bi in range(n):
            stride = 2 if (li > 0 and bi == 0) else 1
            pre = f"layer{li + 1}.{bi}"
            out = planes * block.expansion
            if block is BasicBlock:
                idx = [conv_bn(pre + ".conv1", pre + ".bn1", inplanes, planes, 3, stride, 1),
                       conv_bn(pre + ".conv2", pre + ".bn2", planes, planes, 3, 1, 1)]
            elif block is Bottleneck:
                idx = [conv_bn(pre + ".conv1", pre + ".bn1", inplanes, planes, 1, 1, 0),
                       conv_bn(pre + ".conv2", pre + ".bn2", planes, planes, 3, stride, 1),
                       conv_bn(pre + ".conv3", pre + ".bn3", planes, out, 1, 1, 0)]
            else:
                raise TypeError("block must be resnet.BasicBlock or resnet.Bottleneck")
            ds = None
            if stride != 1 or inplanes != out:
                ds = conv_bn(pre + ".downsample.0", pre + ".downsample.1", inplanes, out, 1, stride, 0)
            blocks.append((pre, idx, ds))
            inplanes = out
    specs["fc.weight"] = (num_classes, inplanes)
    specs["fc.bias"] = (num_classes,)
    return specs, convs, blocks


def _out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def resnet_flops(block, layers, num_classes, H, W):
    """Algorithmic FLOPs of one image: 2 * output pixels * c_out * c_in * k^2 per convolution + the head."""
    specs, convs, blocks = resnet_plan(block, layers, num_classes)
    _, _, cin, cout, k, s, p = convs[0]
    h, w = _out_size(H, k, s, p), _out_size(W, k, s, p)
    total = 2.0 * h * w * cout * cin * k * k
    h, w = _out_size(h, 3, 2, 1), _out_size(w, 3, 2, 1)
    for _, idx, ds in blocks:
        hi, wi = h, w
        for i in idx:
            _, _, cin, cout, k, s, p = convs[i]
            h, w = _out_size(h, k, s, p), _out_size(w, k, s, p)
            total += 2.0 * h * w * cout * cin * k * k
        if ds is not None:
            _, _, cin, cout, k, s, p = convs[ds]
            total += 2.0 * _out_size(hi, k, s, p) * _out_size(wi, k, s, p) * cout * cin
    return total + 2.0 * specs["fc.weight"][0] * specs["fc.weight"][1]


class ResNet(ForwardNet):
    """torchvision's ResNet, forward only: ``model(x)`` takes a normalised fp32 [B, 3, H, W] tensor (what the reference's loader hands to
    the model), ``forward_u8(images, mean, std)`` uint8 [B, H, W, 3] bytes that it normalises on the fly.  Both return fp32 logits
    [B, num_classes] on the device."""

    def __init__(self, block, layers, num_classes=1000, device="cuda", max_chunk_bytes=1 << 30):
        super().__init__(device)
        self.block, self.layers, self.num_classes = block, tuple(layers), int(num_classes)
        self.max_chunk_bytes = int(max_chunk_bytes)
        self.specs, self.convs, self.blocks = resnet_plan(block, layers, num_classes)
        self.feat = self.specs["fc.weight"][1]
        self._loaded = None
        self.training = False

    # ---------------------------------------------------------------- torch.nn.Module's surface, as far as inference goes
    def eval(self):
        return self

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("ResNet is inference only: BatchNorm is folded at load (eval mode)")
        return self

    def to(self, *a, **k):
        return self

    def __call__(self, x):
        return self.forward(x)

    # ---------------------------------------------------------------- weights
    def _canonical(self, sd):
        if "state_dict" in sd and isinstance(sd["state_dict"], dict):
            sd = sd["state_dict"]
        if sd and all(k.startswith("module.") for k in sd):
            sd = OrderedDict((k[len("module."):], v) for k, v in sd.items())
        missing = [n for n in self.specs if n not in sd and not n.endswith("num_batches_tracked")]
        extra = [n for n in sd if n not in self.specs]
        if missing or extra:
            raise KeyError(f"ResNet state dict does not match the architecture: missing keys {missing}, unexpected keys {extra}")
        out = OrderedDict()
        for n, shp in self.specs.items():
            if n not in sd:
                continue
            t = torch.as_tensor(sd[n]).detach().cpu()
            if tuple(t.shape) != tuple(shp):
                raise ValueError(f"{n}: shape {tuple(t.shape)}, the architecture needs {tuple(shp)}")
            out[n] = t.clone()
        return out

    def load_state_dict(self, sd):
        can = self._canonical(sd)                     # raises before anything touches the GPU
        # arena: the folded weights (stem [64][k_pad] in patch-column order, every other kernel OIHW) and biases, then fc
        off, index, host = 0, {}, []

        def put(name, t):
            nonlocal off
            index[name] = off
            host.append((off, t.reshape(-1).to(torch.float32)))
            off = (off + t.numel() + 7) // 8 * 8

        for i, (conv, bn, cin, cout, k, s, p) in enumerate(self.convs):
            w, b = fold_bn(can[conv + ".weight"], can[bn + ".weight"], can[bn + ".bias"], can[bn + ".running_mean"], can[bn + ".running_var"])
            if i == 0:
                ws = torch.zeros(cout, STEM_K_PAD, dtype=torch.float64)
                ws[:, :STEM_K] = w.permute(0, 2, 3, 1).reshape(cout, STEM_K)      # column (kh * 7 + kw) * 3 + c
                w = ws
            put(conv + ".w", w)
            put(conv + ".b", b)
        put("fc.weight", can["fc.weight"].to(torch.float64))
        put("fc.bias", can["fc.bias"].to(torch.float64))
        flat = torch.zeros(off, dtype=torch.float32)
        for o, t in host:
            flat[o:o + t.numel()] = t
        self.index, self.n_total = index, off
        self.params = flat.to(self.dev)
        self.params_bf16 = torch.empty(off, dtype=torch.bfloat16, device=self.dev)
        check(_L().sfron_cast_bf16(ptr(self.params), ptr(self.params_bf16), off, stream_ptr()), "cast_bf16")
        self.conv3 = {}
        for conv, bn, cin, cout, k, s, p in self.convs[1:]:
            if k == 3:
                fwd = torch.zeros(cout * 9 * cin, dtype=torch.bfloat16, device=self.dev)
                check(_L().sfron_conv_wprep(self._p(conv + ".w"), cout, cin, 9, cout, cin, ptr(fwd), None, stream_ptr()), "conv_wprep")
                self.conv3[conv] = fwd
        self._loaded = can
        return self

    def state_dict(self):
        if self._loaded is None:
            raise _lib.SfronError("ResNet.state_dict: no weights loaded")
        return OrderedDict((n, v.clone()) for n, v in self._loaded.items())

    def view(self, name):
        raise NotImplementedError("ResNet.view: the arena holds BatchNorm-folded weights, not the state dict's tensors; use state_dict()")

    # ---------------------------------------------------------------- the 2 GiB rule
    def per_sample_bytes(self, H, W):
        """Bytes of the largest operand one sample contributes to a launch: the input, the stem's patch matrix and fp32 output, the fp32
        activations of every block."""
        h, w = _out_size(H, 7, 2, 3), _out_size(W, 7, 2, 3)
        big = max(H * W * 3 * 4, h * w * STEM_K_PAD * 2, h * w * 64 * 4)
        h, w = _out_size(h, 3, 2, 1), _out_size(w, 3, 2, 1)
        big = max(big, h * w * 64 * 4)
        for _, idx, ds in self.blocks:
            for i in idx:
                _, _, cin, cout, k, s, p = self.convs[i]
                h, w = _out_size(h, k, s, p), _out_size(w, k, s, p)
                big = max(big, h * w * cout * 4)
        return big

    # ---------------------------------------------------------------- launches
    def _conv(self, i, src, B, h, w, out_key, resid=None):
        """Convolution i (+ folded BatchNorm bias, + fp32 residual) of bf16 rows [B * h * w][c_in] -> fp32 rows, and the output size."""
        from .unet import _conv_desc
        conv, _, cin, cout, k, s, p = self.convs[i]
        ho, wo = _out_size(h, k, s, p), _out_size(w, k, s, p)
        out = self._buf(out_key, B * ho * wo * cout, torch.float32)
        guard(src, out, resid)
        d = _conv_desc(B, h, w, cin, ho, wo, cout, k * k, s, p, 0, 0, bias=self._p(conv + ".b"), resid=resid, out_f32=out, ld_out=cout)
        wt = ptr(self.conv3[conv]) if k == 3 else self._w(conv + ".w")
        check(_L().sfron_conv_fwd(ctypes.byref(d), ptr(src), wt, stream_ptr()), f"conv_fwd({conv})")
        return out, ho, wo

    def _relu(self, x, rows, C, bf_key, keep_f32):
        """bf16(max(x, 0)) for the next product; with keep_f32 x itself becomes max(x, 0) too (the next block's residual)."""
        y = self._buf(bf_key, rows * C, torch.bfloat16)
        guard(x, y)
        check(_L().sfron_relu_rows(ptr(x), C, rows, C, ptr(y), ptr(x) if keep_f32 else None, stream_ptr()), "relu_rows")
        return y

    def _chunk(self, images, norm, lo, hi, logits):
        from .unet import bgemm
        L, B = _L(), hi - lo
        src = images[lo:hi]
        if norm is not None:
            H, W = images.shape[1], images.shape[2]
        else:
            H, W = images.shape[2], images.shape[3]
        h, w = _out_size(H, 7, 2, 3), _out_size(W, 7, 2, 3)
        pat = self._buf("bf_patch", B * h * w * STEM_K_PAD, torch.bfloat16)
        guard(src, pat)
        if norm is not None:
            check(L.sfron_image_u8_patches7(ptr(src), B, H, W, *norm, STEM_K_PAD, ptr(pat), stream_ptr()), "image_u8_patches7")
        else:
            check(L.sfron_nchw_patches7(ptr(src), B, H, W, STEM_K_PAD, ptr(pat), stream_ptr()), "nchw_patches7")
        stem = self._buf("f_t", B * h * w * 64, torch.float32)
        guard(stem)
        bgemm(pat, self._w("conv1.w"), B * h * w, 64, STEM_K_PAD, lda=STEM_K_PAD, ldb=STEM_K_PAD, bias=self._p("conv1.b"), c_f32=stem, ldc=64)
        hp, wp = _out_size(h, 3, 2, 1), _out_size(w, 3, 2, 1)
        xf = self._buf("f_x0", B * hp * wp * 64, torch.float32)
        xb = self._buf("bf_x0", B * hp * wp * 64, torch.bfloat16)
        check(L.sfron_relu_maxpool3s2(ptr(stem), 64, B, h, w, 64, 1, ptr(xb), ptr(xf), stream_ptr()), "relu_maxpool3s2")
        h, w, C, cur = hp, wp, 64, 0
        for _, idx, ds in self.blocks:
            t, th, tw = xb, h, w
            for j, i in enumerate(idx[:-1]):
                o, th, tw = self._conv(i, t, B, th, tw, "f_t")
                t = self._relu(o, B * th * tw, self.convs[i][3], f"bf_t{j}", False)
            sc = xf if ds is None else self._conv(ds, xb, B, h, w, "f_sc")[0]
            nxt = 1 - cur
            xf, h, w = self._conv(idx[-1], t, B, th, tw, f"f_x{nxt}", resid=sc)
            C = self.convs[idx[-1]][3]
            xb = self._relu(xf, B * h * w, C, f"bf_x{nxt}", True)
            cur = nxt
        pooled = self._buf("f_pool", B * C, torch.float32)
        check(L.sfron_pool_fc(ptr(xf), C, B, h * w, C, self._p("fc.weight"), self._p("fc.bias"), self.num_classes, ptr(pooled),
                              logits.data_ptr() + 4 * lo * self.num_classes, stream_ptr()), "pool_fc")

    def _run(self, images, norm):
        if self._loaded is None:
            raise _lib.SfronError("ResNet: load_state_dict first")
        B = images.shape[0]
        H, W = (images.shape[1], images.shape[2]) if norm is not None else (images.shape[2], images.shape[3])
        logits = torch.empty(B, self.num_classes, dtype=torch.float32, device=self.dev)
        n = self.chunk_size(H, W)
        for lo in range(0, B, n):
            self._chunk(images, norm, lo, min(B, lo + n), logits)
        return logits

    @torch.no_grad()
    def forward(self, x):
        """fp32 logits of a normalised fp32 [B, 3, H, W] batch (host or device)."""
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[0] < 1:
            raise ValueError(f"ResNet takes [B, 3, H, W], got {tuple(x.shape)}")
        return self._run(x.to(self.dev, torch.float32).contiguous(), None)

    @torch.no_grad()
    def forward_u8(self, images_u8_nhwc, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)):
        """fp32 logits of uint8 [B, H, W, 3] images: ToTensor + Normalize(mean, std) happen inside the stem's patch kernel."""
        x = images_u8_nhwc
        if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3 or x.shape[0] < 1:
            raise ValueError(f"forward_u8 takes uint8 [B, H, W, 3], got {x.dtype} {tuple(x.shape)}")
        mean, std = [float(np.float32(v)) for v in mean], [float(np.float32(v)) for v in std]
        if len(mean) != 3 or len(std) != 3 or any(s == 0.0 for s in std):
            raise ValueError("mean and std: three values, std non-zero")
        return self._run(x.to(self.dev).contiguous(), tuple(mean) + tuple(std))


def resnet34(num_classes=1000, **kw):
    return ResNet(BasicBlock, [3, 4, 6, 3], num_classes=num_classes, **kw)


def resnet50(num_classes=1000, **kw):
    return ResNet(Bottleneck, [3, 4, 6, 3], num_classes=num_classes, **kw)

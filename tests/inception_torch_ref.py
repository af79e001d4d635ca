"""The FID Inception-v3 (``pt_inception-2015-12-05`` of pytorch-fid / torch-fidelity: the 2015 TF Inception under torchvision's names)
restated in plain torch.nn with the published state_dict key names: the yardstick of sfron.inception on the CPU.  None of those libraries
is part of this project's environment, so parity at that boundary is unpinned.

The three FID variants are constructor switches so that the tests can turn each off and see the distance: ``count_include_pad`` (False in
the FID net: the 3x3 stride-1 average pools of the A, C and E blocks divide by the in-bounds count), ``last_pool`` ("max" in the FID net:
Mixed_7c's pool branch) and ``resize`` ("tf1": src = dst * in / out, no half-pixel offset, the neighbour clamped; "half_pixel" is
F.interpolate's rule).

Beside the fp32 model: ``randomize`` (the seeded weights of the tests), ``Emulated`` (the same network with BatchNorm folded and every
convolution input rounded to bf16 -- what the GPU path computes, up to the accumulation order) and ``rel_l2``."""
import torch
import torch.nn as nn
import torch.nn.functional as F

SIZE = 299
TAPS = (64, 192, 768, 2048)


class BasicConv2d(nn.Module):
    def __init__(self, cin, cout, **kw):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, bias=False, **kw)
        self.bn = nn.BatchNorm2d(cout, eps=0.001)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)))


def _avg(x, count_include_pad):
    return F.avg_pool2d(x, 3, 1, 1, count_include_pad=count_include_pad)


class InceptionA(nn.Module):
    def __init__(self, cin, pool_features, cip):
        super().__init__()
        self.cip = cip
        self.branch1x1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch5x5_1 = BasicConv2d(cin, 48, kernel_size=1)
        self.branch5x5_2 = BasicConv2d(48, 64, kernel_size=5, padding=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, padding=1)
        self.branch_pool = BasicConv2d(cin, pool_features, kernel_size=1)

    def forward(self, x, cv):
        return torch.cat([cv(self.branch1x1, x), cv(self.branch5x5_2, cv(self.branch5x5_1, x)),
                          cv(self.branch3x3dbl_3, cv(self.branch3x3dbl_2, cv(self.branch3x3dbl_1, x))),
                          cv(self.branch_pool, _avg(x, self.cip))], 1)


class InceptionB(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3 = BasicConv2d(cin, 384, kernel_size=3, stride=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, stride=2)

    def forward(self, x, cv):
        return torch.cat([cv(self.branch3x3, x), cv(self.branch3x3dbl_3, cv(self.branch3x3dbl_2, cv(self.branch3x3dbl_1, x))),
                          F.max_pool2d(x, 3, 2)], 1)


class InceptionC(nn.Module):
    def __init__(self, cin, c7, cip):
        super().__init__()
        self.cip = cip
        self.branch1x1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch7x7_1 = BasicConv2d(cin, c7, kernel_size=1)
        self.branch7x7_2 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7_3 = BasicConv2d(c7, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = BasicConv2d(cin, c7, kernel_size=1)
        self.branch7x7dbl_2 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = BasicConv2d(c7, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch_pool = BasicConv2d(cin, 192, kernel_size=1)

    def forward(self, x, cv):
        b7 = cv(self.branch7x7_3, cv(self.branch7x7_2, cv(self.branch7x7_1, x)))
        bd = cv(self.branch7x7dbl_1, x)
        for m in (self.branch7x7dbl_2, self.branch7x7dbl_3, self.branch7x7dbl_4, self.branch7x7dbl_5):
            bd = cv(m, bd)
        return torch.cat([cv(self.branch1x1, x), b7, bd, cv(self.branch_pool, _avg(x, self.cip))], 1)


class InceptionD(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3_1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch3x3_2 = BasicConv2d(192, 320, kernel_size=3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch7x7x3_2 = BasicConv2d(192, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(192, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(192, 192, kernel_size=3, stride=2)

    def forward(self, x, cv):
        b7 = cv(self.branch7x7x3_1, x)
        for m in (self.branch7x7x3_2, self.branch7x7x3_3, self.branch7x7x3_4):
            b7 = cv(m, b7)
        return torch.cat([cv(self.branch3x3_2, cv(self.branch3x3_1, x)), b7, F.max_pool2d(x, 3, 2)], 1)


class InceptionE(nn.Module):
    def __init__(self, cin, pool, cip):
        super().__init__()
        self.pool, self.cip = pool, cip
        self.branch1x1 = BasicConv2d(cin, 320, kernel_size=1)
        self.branch3x3_1 = BasicConv2d(cin, 384, kernel_size=1)
        self.branch3x3_2a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3_2b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(cin, 448, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(448, 384, kernel_size=3, padding=1)
        self.branch3x3dbl_3a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(cin, 192, kernel_size=1)

    def forward(self, x, cv):
        b3 = cv(self.branch3x3_1, x)
        bd = cv(self.branch3x3dbl_2, cv(self.branch3x3dbl_1, x))
        p = F.max_pool2d(x, 3, 1, 1) if self.pool == "max" else _avg(x, self.cip)
        return torch.cat([cv(self.branch1x1, x), cv(self.branch3x3_2a, b3), cv(self.branch3x3_2b, b3), cv(self.branch3x3dbl_3a, bd),
                          cv(self.branch3x3dbl_3b, bd), cv(self.branch_pool, p)], 1)


def resize_tf1(x, size=SIZE, dtype=torch.float32):
    """TF1's legacy bilinear resize of [B, C, H, W] values: src = dst * in / out, lo = floor, hi = min(lo + 1, in - 1), in ``dtype``."""
    x = x.to(dtype)
    H, W = x.shape[2], x.shape[3]

    def axis(n_in):
        src = torch.arange(size, dtype=dtype) * (torch.tensor(n_in, dtype=dtype) / torch.tensor(size, dtype=dtype))
        lo = src.floor().long().clamp(max=n_in - 1)
        return lo, (lo + 1).clamp(max=n_in - 1), src - lo.to(dtype)

    y0, y1, fy = axis(H)
    x0, x1, fx = axis(W)
    top, bot = x[:, :, y0, :], x[:, :, y1, :]
    top = top[..., x0] + (top[..., x1] - top[..., x0]) * fx
    bot = bot[..., x0] + (bot[..., x1] - bot[..., x0]) * fx
    return top + (bot - top) * fy.view(-1, 1)


class FIDInceptionV3(nn.Module):
    def __init__(self, count_include_pad=False, last_pool="max", resize="tf1"):
        super().__init__()
        cip = count_include_pad
        self.resize = resize
        self.Conv2d_1a_3x3 = BasicConv2d(3, 32, kernel_size=3, stride=2)
        self.Conv2d_2a_3x3 = BasicConv2d(32, 32, kernel_size=3)
        self.Conv2d_2b_3x3 = BasicConv2d(32, 64, kernel_size=3, padding=1)
        self.Conv2d_3b_1x1 = BasicConv2d(64, 80, kernel_size=1)
        self.Conv2d_4a_3x3 = BasicConv2d(80, 192, kernel_size=3)
        self.Mixed_5b = InceptionA(192, 32, cip)
        self.Mixed_5c = InceptionA(256, 64, cip)
        self.Mixed_5d = InceptionA(288, 64, cip)
        self.Mixed_6a = InceptionB(288)
        self.Mixed_6b = InceptionC(768, 128, cip)
        self.Mixed_6c = InceptionC(768, 160, cip)
        self.Mixed_6d = InceptionC(768, 160, cip)
        self.Mixed_6e = InceptionC(768, 192, cip)
        self.Mixed_7a = InceptionD(768)
        self.Mixed_7b = InceptionE(1280, "avg", cip)
        self.Mixed_7c = InceptionE(2048, last_pool, cip)
        self.fc = nn.Linear(2048, 1008)

    def blocks(self):
        return [getattr(self, n) for n in ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e",
                                           "Mixed_7a", "Mixed_7b", "Mixed_7c")]

    def preprocess(self, images_u8_nhwc):
        x = images_u8_nhwc.permute(0, 3, 1, 2).float()
        if self.resize == "tf1":
            x = resize_tf1(x)
        else:
            x = F.interpolate(x, size=(SIZE, SIZE), mode="bilinear", align_corners=False)
        return (x - 128.0) / 128.0

    def taps(self, images_u8_nhwc, cv=None, widths=False, upto=2048):
        """{tap width: [B, width]} of uint8 [B, H, W, 3] images, the taps up to ``upto``; ``cv(module, x)`` runs one conv + bn + relu
        (default: the module); with ``widths`` also the channel count after every block."""
        cv = cv or (lambda m, x: m(x))
        out, ws = {}, []
        x = self.preprocess(images_u8_nhwc)
        x = cv(self.Conv2d_2b_3x3, cv(self.Conv2d_2a_3x3, cv(self.Conv2d_1a_3x3, x)))
        x = F.max_pool2d(x, 3, 2)
        out[64] = x.mean(dim=(2, 3))
        if upto <= 64:
            return out
        x = cv(self.Conv2d_4a_3x3, cv(self.Conv2d_3b_1x1, x))
        x = F.max_pool2d(x, 3, 2)
        out[192] = x.mean(dim=(2, 3))
        if upto <= 192:
            return out
        for blk in self.blocks():
            x = blk(x, cv)
            ws.append(x.shape[1])
            if blk is self.Mixed_6e:
                out[768] = x.mean(dim=(2, 3))
                if upto <= 768:
                    return out
        out[2048] = x.mean(dim=(2, 3))
        return (out, ws) if widths else out

    @torch.no_grad()
    def forward(self, images_u8_nhwc, upto=2048):
        return self.taps(images_u8_nhwc, upto=upto)


def randomize(model, seed, probe=None):
    """Seeded weights: Kaiming fan-in convolutions (std sqrt(2 / fan_in): a ReLU layer then keeps the second moment of its input), BN
    gamma ~ U(0.5, 1.5), beta and running_mean ~ N(0, 0.1), running_var ~ U(0.5, 1.5).  With ``probe`` (uint8 images) the draw is checked:
    at every tap the deviation of the features over the probe must lie in [0.02, 50] -- activations neither die nor grow through the depth."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.Conv2d):
                fan_in = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
            elif isinstance(m, nn.BatchNorm2d):
                n = m.weight.shape[0]
                m.weight.copy_(torch.rand(n, generator=g) + 0.5)
                m.bias.copy_(torch.randn(n, generator=g) * 0.1)
                m.running_mean.copy_(torch.randn(n, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(n, generator=g) + 0.5)
            elif isinstance(m, nn.Linear):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (1.0 / m.weight.shape[1]) ** 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
        model.eval()
        if probe is not None:
            for t, f in model(probe).items():
                dev = float(f.std())
                assert 0.02 <= dev <= 50.0, f"tap {t}: feature deviation {dev}"
    return model


def _bf(t):
    return t.to(torch.bfloat16).to(torch.float32)


class Emulated:
    """The fp32 restatement with what the GPU path does to the numbers: BatchNorm folded into the convolution in fp64 (w' = w * s, b' = beta -
    mean * s, s = gamma / sqrt(var + 1e-3)), w' and every convolution INPUT rounded to bf16 (the resized, normalised input included), fp32
    accumulation and bias, ReLU, pools and feature taps on the unrounded fp32 values."""

    def __init__(self, model):
        self.m = model.eval()
        self._folded = {}

    def _cv(self, mod, x):
        if mod not in self._folded:
            conv, bn = mod.conv, mod.bn
            s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
            self._folded[mod] = (_bf((conv.weight.double() * s.view(-1, 1, 1, 1)).float()), (bn.bias.double() - bn.running_mean.double() * s).float())
        w, b = self._folded[mod]
        return F.relu(F.conv2d(_bf(x), w, b, mod.conv.stride, mod.conv.padding))

    @torch.no_grad()
    def __call__(self, images_u8_nhwc, upto=2048):
        return self.m.taps(images_u8_nhwc, self._cv, upto=upto)


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())

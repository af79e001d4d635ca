"""torchvision's published ResNet (v1.5) restated in plain torch.nn with torchvision's state_dict key names: the yardstick of sfron.resnet
on the CPU.  torchvision itself is not part of this project's environment, so parity at that boundary is unpinned.

Beside the fp32 model: ``randomize`` (the seeded weights of the tests), ``Emulated`` (the same network with BatchNorm folded and every
convolution input rounded to bf16 -- what the GPU path computes, up to the accumulation order) and ``rel_l2``."""
import torch
import torch.nn as nn
import torch.nn.functional as F


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.relu(out + identity)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)          # v1.5: the stride sits on the 3x3
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.relu(out + identity)


class ResNet(nn.Module):
    def __init__(self, block, layers, num_classes=1000):
        super().__init__()
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], 2)
        self.layer3 = self._make_layer(block, 256, layers[2], 2)
        self.layer4 = self._make_layer(block, 512, layers[3], 2)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512 * block.expansion, num_classes)

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * block.expansion, 1, stride, bias=False),
                                       nn.BatchNorm2d(planes * block.expansion))
        layers = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        layers += [block(self.inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    def features(self, x):
        """the pooled features [B, C] the head reads"""
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return torch.flatten(self.avgpool(x), 1)

    def forward(self, x):
        return self.fc(self.features(x))


def resnet34(num_classes=1000):
    return ResNet(BasicBlock, [3, 4, 6, 3], num_classes)


def resnet50(num_classes=1000):
    return ResNet(Bottleneck, [3, 4, 6, 3], num_classes)


def randomize(model, seed, logit_cap=None, probe=None):
    """Seeded weights: Kaiming fan-out convolutions, BN gamma ~ U(0.5, 1.5), beta and running_mean ~ N(0, 0.1), running_var ~ U(0.5, 1.5).
    With ``logit_cap`` and ``probe`` batches ``fc.weight`` is scaled so that |logit| <= logit_cap on every probe (bias zero)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.Conv2d):
                fan_out = m.weight.shape[0] * m.weight.shape[2] * m.weight.shape[3]
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_out) ** 0.5)
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
        if logit_cap is not None:
            model.fc.bias.zero_()
            top = max(float(model(p).abs().max()) for p in probe)
            if top > logit_cap:
                model.fc.weight.mul_(logit_cap / top * (1 - 1e-6))
    return model


def _bf(t):
    return t.to(torch.bfloat16).to(torch.float32)


class Emulated:
    """The fp32 restatement with what the GPU path does to the numbers: BatchNorm folded into the convolution in fp64 (w' = w * s, b' = beta -
    mean * s, s = gamma / sqrt(var + 1e-5)), w' and every convolution INPUT rounded to bf16, fp32 accumulation, fp32 bias / residual / head."""

    def __init__(self, model):
        self.m = model.eval()

    @staticmethod
    def _conv(x, conv, bn):
        s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        w = (conv.weight.double() * s.view(-1, 1, 1, 1)).float()
        b = (bn.bias.double() - bn.running_mean.double() * s).float()
        return F.conv2d(_bf(x), _bf(w), b, conv.stride, conv.padding)

    def _block(self, blk, x):
        identity = x if blk.downsample is None else self._conv(x, blk.downsample[0], blk.downsample[1])
        out = F.relu(self._conv(x, blk.conv1, blk.bn1))
        if isinstance(blk, Bottleneck):
            out = F.relu(self._conv(out, blk.conv2, blk.bn2))
            out = self._conv(out, blk.conv3, blk.bn3)
        else:
            out = self._conv(out, blk.conv2, blk.bn2)
        return F.relu(out + identity)

    @torch.no_grad()
    def features(self, x):
        m = self.m
        x = F.max_pool2d(F.relu(self._conv(x, m.conv1, m.bn1)), 3, 2, 1)
        for layer in (m.layer1, m.layer2, m.layer3, m.layer4):
            for blk in layer:
                x = self._block(blk, x)
        return x.mean(dim=(2, 3))

    @torch.no_grad()
    def __call__(self, x):
        return self.m.fc(self.features(x))


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())

"""The FID Inception-v3 over the HIP kernels of csrc/inception.hip, csrc/conv.hip and csrc/classify.hip, forward only.

Restates the network pytorch-fid and torch-fidelity publish as ``pt_inception-2015-12-05`` -- the 2015 TF Inception the ADM evaluator's
graph (DDPM/evaluator.py) holds, under torchvision's ``Inception3`` names -- with that file's ``state_dict`` keys.  None of those libraries
is part of this project's environment: the architecture, its three FID variants and the resize rule are restated from their published
text, so parity at that boundary is unpinned.  The variants: the 3x3 stride-1 average pools of the A, C and E blocks
do not count padding; ``Mixed_7c`` pools with a maximum in its pool branch; the input is ``(x - 128) / 128`` of the bytes resized to
299 x 299 by TF1's legacy bilinear rule (``src = dst * in / out``, no half-pixel offset, the neighbour index clamped).

``inception_plan`` states the network once: keys and shapes, the convolution list, the block list.  BatchNorm (eps 1e-3) is folded into the
convolution before it at load, in fp64 on the host (``resnet.fold_bn``).  Activations are NHWC rows.  The 1x1 convolutions and the 3x3
ones with one symmetric pad are sfron_conv_fwd; 1x7, 7x1, 1x3, 3x1, 5x5 and the first convolution (3 input channels, padded to 8 by the
resize kernel) are a patch matrix (sfron_patch_rows) times the weights on the batched GEMM, as the ResNet stem.  The last product of a
branch writes its fp32 columns straight into the block's concatenated row (``ld_out`` / ``ldc`` = block width): no concat pass runs.

ReLU is sfron_relu_rows, the row kernel that also casts to bf16 for the next product, once over a block's whole concatenated row: the
products keep their epilogues (a new epilogue value would touch every GEMM instantiation for one compare per value), the bf16 cast is
needed anyway, and the fp32 row it leaves in place is what the average pools and the feature taps read -- so the pools see unrounded
values, as in the fp32 network.

Chunk invariant (forward_net.py): a batch runs in chunks of samples whose largest operand stays under ``max_chunk_bytes``; every launch
asserts its operands are below 2 GiB.
"""
import ctypes
from collections import OrderedDict

import torch

from . import _lib
from ._lib import check, lib as _L, ptr, stream_ptr
from .forward_net import ForwardNet, guard
from .resnet import fold_bn

BN_EPS = 1e-3
SIZE = 299                   # the network's input is always SIZE x SIZE
C_PAD = 8                    # channels of the resized input rows: 3 live, 5 zero
TAPS = (64, 192, 768, 2048)
BLOCK_WIDTHS = (256, 288, 288, 768, 768, 768, 768, 768, 1280, 2048, 2048)
FC_OUT = 1008


def _out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def inception_plan():
    """(specs, convs, stem, blocks).  ``specs`` {state_dict key: shape} in the published order (``fc.*`` last); ``convs`` [(name, c_in,
    c_out, kh, kw, stride, pad_h, pad_w)] (keys ``name.conv.weight``, ``name.bn.*``); ``stem`` the steps before the blocks; ``blocks``
    [(name, c_in, width, branches)] where a branch is a tuple of steps whose last one writes the next columns of the concatenated row.
    Steps: ("conv", i), ("avg",) / ("max1",) = 3x3 stride-1 pad-1 pools, ("max2",) = MaxPool(3, 2), ("fork", i, j) = two convolutions of
    the same input side by side, ("tap", width) = a feature tap (stem only; the taps 768 and 2048 follow Mixed_6e and Mixed_7c)."""
    specs, convs = OrderedDict(), []

    def cv(name, cin, cout, k, stride=1, pad=0):
        kh, kw = (k, k) if isinstance(k, int) else k
        ph, pw = (pad, pad) if isinstance(pad, int) else pad
        specs[name + ".conv.weight"] = (cout, cin, kh, kw)
        for n in ("weight", "bias", "running_mean", "running_var"):
            specs[f"{name}.bn.{n}"] = (cout,)
        specs[name + ".bn.num_batches_tracked"] = ()
        convs.append((name, cin, cout, kh, kw, stride, ph, pw))
        return ("conv", len(convs) - 1)

    stem = [cv("Conv2d_1a_3x3", 3, 32, 3, 2), cv("Conv2d_2a_3x3", 32, 32, 3), cv("Conv2d_2b_3x3", 32, 64, 3, 1, 1), ("max2",), ("tap", 64),
            cv("Conv2d_3b_1x1", 64, 80, 1), cv("Conv2d_4a_3x3", 80, 192, 3), ("max2",), ("tap", 192)]
    blocks = []

    def block_a(name, cin, pf):
        p = name + "."
        br = [(cv(p + "branch1x1", cin, 64, 1),),
              (cv(p + "branch5x5_1", cin, 48, 1), cv(p + "branch5x5_2", 48, 64, 5, 1, 2)),
              (cv(p + "branch3x3dbl_1", cin, 64, 1), cv(p + "branch3x3dbl_2", 64, 96, 3, 1, 1), cv(p + "branch3x3dbl_3", 96, 96, 3, 1, 1))]
        br.append((("avg",), cv(p + "branch_pool", cin, pf, 1)))
        blocks.append((name, cin, 224 + pf, br))

    def block_b(name, cin):
        p = name + "."
        br = [(cv(p + "branch3x3", cin, 384, 3, 2),),
              (cv(p + "branch3x3dbl_1", cin, 64, 1), cv(p + "branch3x3dbl_2", 64, 96, 3, 1, 1), cv(p + "branch3x3dbl_3", 96, 96, 3, 2)),
              (("max2",),)]
        blocks.append((name, cin, 480 + cin, br))

    def block_c(name, cin, c7):
        p = name + "."
        br = [(cv(p + "branch1x1", cin, 192, 1),),
              (cv(p + "branch7x7_1", cin, c7, 1), cv(p + "branch7x7_2", c7, c7, (1, 7), 1, (0, 3)), cv(p + "branch7x7_3", c7, 192, (7, 1), 1, (3, 0))),
              (cv(p + "branch7x7dbl_1", cin, c7, 1), cv(p + "branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0)),
               cv(p + "branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3)), cv(p + "branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0)),
               cv(p + "branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3)))]
        br.append((("avg",), cv(p + "branch_pool", cin, 192, 1)))
        blocks.append((name, cin, 768, br))

    def block_d(name, cin):
        p = name + "."
        br = [(cv(p + "branch3x3_1", cin, 192, 1), cv(p + "branch3x3_2", 192, 320, 3, 2)),
              (cv(p + "branch7x7x3_1", cin, 192, 1), cv(p + "branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3)),
               cv(p + "branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0)), cv(p + "branch7x7x3_4", 192, 192, 3, 2)),
              (("max2",),)]
        blocks.append((name, cin, 512 + cin, br))

    def block_e(name, cin, pool):
        p = name + "."
        b1 = (cv(p + "branch1x1", cin, 320, 1),)
        c1, ca, cb = cv(p + "branch3x3_1", cin, 384, 1), cv(p + "branch3x3_2a", 384, 384, (1, 3), 1, (0, 1)), cv(p + "branch3x3_2b", 384, 384, (3, 1), 1, (1, 0))
        b2 = (c1, ("fork", ca[1], cb[1]))
        d1, d2 = cv(p + "branch3x3dbl_1", cin, 448, 1), cv(p + "branch3x3dbl_2", 448, 384, 3, 1, 1)
        da, db = cv(p + "branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1)), cv(p + "branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0))
        b3 = (d1, d2, ("fork", da[1], db[1]))
        b4 = ((pool,), cv(p + "branch_pool", cin, 192, 1))
        blocks.append((name, cin, 2048, [b1, b2, b3, b4]))

    block_a("Mixed_5b", 192, 32)
    block_a("Mixed_5c", 256, 64)
    block_a("Mixed_5d", 288, 64)
    block_b("Mixed_6a", 288)
    for name, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        block_c(name, 768, c7)
    block_d("Mixed_7a", 768)
    block_e("Mixed_7b", 1280, "avg")
    block_e("Mixed_7c", 2048, "max1")          # the FID variant: a max pool in the last block's pool branch
    specs["fc.weight"] = (FC_OUT, 2048)
    specs["fc.bias"] = (FC_OUT,)
    return specs, convs, stem, blocks


def _walk(convs, stem, blocks, on_conv, upto=2048):
    """Calls on_conv(i, h, w, ho, wo) for every convolution up to the tap ``upto`` at a SIZE x SIZE input (shape bookkeeping shared by
    ``flops`` and ``per_sample_bytes``)."""
    h = w = SIZE

    def conv(i, h, w):
        _, _, _, kh, kw, s, ph, pw = convs[i]
        ho, wo = _out_size(h, kh, s, ph), _out_size(w, kw, s, pw)
        on_conv(i, h, w, ho, wo)
        return ho, wo

    for st in stem:
        if st[0] == "conv":
            h, w = conv(st[1], h, w)
        elif st[0] == "max2":
            h, w = _out_size(h, 3, 2, 0), _out_size(w, 3, 2, 0)
        elif st[1] >= upto:
            return
    for name, cin, width, branches in blocks:
        for br in branches:
            th, tw = h, w
            for st in br:
                if st[0] == "conv":
                    th, tw = conv(st[1], th, tw)
                elif st[0] == "fork":
                    conv(st[1], th, tw)
                    th, tw = conv(st[2], th, tw)
                elif st[0] == "max2":
                    th, tw = _out_size(th, 3, 2, 0), _out_size(tw, 3, 2, 0)
        h, w = th, tw
        if name == "Mixed_6e" and upto <= 768:
            return


def flops(upto=2048):
    """Algorithmic FLOPs of one image up to the tap ``upto``: 2 * output pixels * c_out * c_in * kh * kw per convolution."""
    specs, convs, stem, blocks = inception_plan()
    total = [0.0]

    def add(i, h, w, ho, wo):
        _, cin, cout, kh, kw, _, _, _ = convs[i]
        total[0] += 2.0 * ho * wo * cout * cin * kh * kw

    _walk(convs, stem, blocks, add, upto)
    return total[0]


def _direct(cv):
    """True when sfron_conv_fwd takes this convolution: square 1x1 or 3x3 with one symmetric pad, channels a multiple of 8."""
    _, cin, _, kh, kw, _, ph, pw = cv
    return kh == kw and kh in (1, 3) and ph == pw and cin % 8 == 0


class InceptionV3(ForwardNet):
    """``forward_u8(images)``: uint8 [B, H, W, 3] images of any size -> {tap width: fp32 [B, width]} on the device, for the taps asked."""

    def __init__(self, device="cuda", max_chunk_bytes=1 << 30):
        super().__init__(device)
        self.max_chunk_bytes = int(max_chunk_bytes)
        self.specs, self.convs, self.stem, self.blocks = inception_plan()
        self._loaded = None
        self.fc_weight = None        # fp32 [1008][2048] on the device once a state dict with fc.weight is loaded
        self.training = False

    def eval(self):
        return self

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("InceptionV3 is inference only: BatchNorm is folded at load (eval mode)")
        return self

    def to(self, *a, **k):
        return self

    # ---------------------------------------------------------------- weights
    def _canonical(self, sd):
        """-> (the tensors the extractor needs, ``fc.weight`` or None); ``fc.*`` is optional."""
        if "state_dict" in sd and isinstance(sd["state_dict"], dict):
            sd = sd["state_dict"]
        need = [n for n in self.specs if not n.startswith("fc.") and not n.endswith("num_batches_tracked")]
        missing = [n for n in need if n not in sd]
        extra = [n for n in sd if n not in self.specs]
        if missing or extra:
            raise KeyError(f"Inception state dict does not match the architecture: missing keys {missing}, unexpected keys {extra}")
        out = OrderedDict()
        for n in need + [n for n in ("fc.weight",) if n in sd]:
            t = torch.as_tensor(sd[n]).detach().cpu()
            if tuple(t.shape) != tuple(self.specs[n]):
                raise ValueError(f"{n}: shape {tuple(t.shape)}, the architecture needs {tuple(self.specs[n])}")
            out[n] = t.clone()
        return out, out.pop("fc.weight", None)

    def load_state_dict(self, sd):
        """Takes the published file's keys.  ``fc.*`` (the 1008-way head, not used by FID) stays optional; when ``fc.weight`` is there it
        is kept as an fp32 device tensor [1008][2048] (not cast to bf16) for ``logits``.  ``fc.bias`` is never used: the reference's
        ``_create_softmax_graph`` multiplies the pooled features by the head's weight matrix (``matmul.inputs[1]``) and adds no bias."""
        can, fc = self._canonical(sd)                 # raises before anything touches the GPU
        off, index, host = 0, {}, []

        def put(name, t):
            nonlocal off
            index[name] = off
            host.append((off, t.reshape(-1).to(torch.float32)))
            off = (off + t.numel() + 7) // 8 * 8

        for i, cv in enumerate(self.convs):
            name, cin, cout, kh, kw = cv[:5]
            w, b = fold_bn(can[name + ".conv.weight"], can[name + ".bn.weight"], can[name + ".bn.bias"], can[name + ".bn.running_mean"],
                           can[name + ".bn.running_var"], eps=BN_EPS)
            if not _direct(cv):                       # patch-matrix order: column (i * kw + j) * c_pad + c
                cp = (cin + 7) // 8 * 8
                ws = torch.zeros(cout, kh, kw, cp, dtype=torch.float64)
                ws[..., :cin] = w.permute(0, 2, 3, 1)
                w = ws
            put(name + ".w", w)
            put(name + ".b", b)
        flat = torch.zeros(off, dtype=torch.float32)
        for o, t in host:
            flat[o:o + t.numel()] = t
        self.index, self.n_total = index, off
        self.params = flat.to(self.dev)
        self.params_bf16 = torch.empty(off, dtype=torch.bfloat16, device=self.dev)
        check(_L().sfron_cast_bf16(ptr(self.params), ptr(self.params_bf16), off, stream_ptr()), "cast_bf16")
        self.conv3 = {}
        for cv in self.convs:
            name, cin, cout, kh = cv[:4]
            if _direct(cv) and kh == 3:
                fwd = torch.zeros(cout * 9 * cin, dtype=torch.bfloat16, device=self.dev)
                check(_L().sfron_conv_wprep(self._p(name + ".w"), cout, cin, 9, cout, cin, ptr(fwd), None, stream_ptr()), "conv_wprep")
                self.conv3[name] = fwd
        self.fc_weight = None if fc is None else fc.to(torch.float32).contiguous().to(self.dev)
        self._loaded = can
        return self

    def logits(self, features_2048):
        """The 1008-way head without its bias over pooled features fp32 [n][2048] on the device: sfron_gemm_nt_f32 against ``fc.weight``
        (exact fp32 products summed in one fixed blocked order per logit) -> fp32 [n][1008]."""
        if self.fc_weight is None:
            raise _lib.SfronError("InceptionV3.logits: the loaded state dict has no fc.weight (the Inception Score needs the 1008-way head)")
        x = features_2048
        if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != 2048 or x.shape[0] < 1:
            raise _lib.SfronError("InceptionV3.logits takes fp32 [n][2048] features on the GPU (no CPU fallback)")
        x = x.contiguous()
        out = torch.empty(x.shape[0], FC_OUT, dtype=torch.float32, device=x.device)
        guard(x, out)
        check(_L().sfron_gemm_nt_f32(ptr(x), x.shape[0], 2048, ptr(self.fc_weight), FC_OUT, 2048, 2048, ptr(out), FC_OUT, stream_ptr()), "gemm_nt_f32")
        return out

    def state_dict(self):
        if self._loaded is None:
            raise _lib.SfronError("InceptionV3.state_dict: no weights loaded")
        return OrderedDict((n, v.clone()) for n, v in self._loaded.items())

    def view(self, name):
        raise NotImplementedError("InceptionV3.view: the arena holds BatchNorm-folded weights, not the state dict's tensors; use state_dict()")

    # ---------------------------------------------------------------- the 2 GiB rule
    def per_sample_bytes(self, H, W):
        """Bytes of the largest operand one sample contributes to a launch: its input bytes, the resized rows, and per convolution the
        patch matrix and the fp32 rows it writes into (a block's whole concatenated row for a branch's last product)."""
        big = [max(H * W * 3, SIZE * SIZE * C_PAD * 2)]
        width_of = {}
        for _, _, width, branches in self.blocks:
            for br in branches:
                for i in (br[-1][1:] if br[-1][0] in ("conv", "fork") else ()):
                    width_of[i] = width

        def see(i, h, w, ho, wo):
            cv = self.convs[i]
            cin, cout, kh, kw = cv[1:5]
            big[0] = max(big[0], ho * wo * max(cout, width_of.get(i, 0)) * 4, h * w * max(cin, C_PAD) * 4)
            if not _direct(cv):
                big[0] = max(big[0], ho * wo * kh * kw * max(cin, C_PAD) * 2)

        _walk(self.convs, self.stem, self.blocks, see)
        return big[0]

    # ---------------------------------------------------------------- launches
    def _conv(self, i, src, B, h, w, dst, ld, keep):
        """Convolution i (+ folded BatchNorm bias) of dense bf16 rows ``src`` -> fp32 at device address ``dst`` with leading dimension
        ``ld``; ``keep`` is the tensor ``dst`` lies in.  Returns the output size."""
        from .unet import _conv_desc, bgemm
        cv = self.convs[i]
        name, cin, cout, kh, kw, s, ph, pw = cv
        ho, wo = _out_size(h, kh, s, ph), _out_size(w, kw, s, pw)
        guard(src, keep)
        if _direct(cv):
            d = _conv_desc(B, h, w, cin, ho, wo, cout, kh * kw, s, ph, 0, 0, bias=self._p(name + ".b"), out_f32=dst, ld_out=ld)
            d.split_ws, d.split_ws_slabs = None, 0        # no split-K: its slab count follows the batch; a sample's features must not
            wt = ptr(self.conv3[name]) if kh == 3 else self._w(name + ".w")
            check(_L().sfron_conv_fwd(ctypes.byref(d), ptr(src), wt, stream_ptr()), f"conv_fwd({name})")
        else:
            cp = max(cin, C_PAD)
            K = kh * kw * cp
            pat = self._buf("bf_patch", B * ho * wo * K, torch.bfloat16)
            guard(pat)
            check(_L().sfron_patch_rows(ptr(src), cp, B, h, w, cp, kh, kw, s, ph, pw, ptr(pat), stream_ptr()), f"patch_rows({name})")
            bgemm(pat, self._w(name + ".w"), B * ho * wo, cout, K, lda=K, ldb=K, bias=self._p(name + ".b"), c_f32=dst, ldc=ld)
        return ho, wo

    def _relu(self, x, rows, C, bf_key, keep_f32=False):
        """bf16(max(x, 0)) of dense fp32 rows for the next product; with keep_f32 x itself becomes max(x, 0) too."""
        y = self._buf(bf_key, rows * C, torch.bfloat16)
        guard(x, y)
        check(_L().sfron_relu_rows(ptr(x), C, rows, C, ptr(y), ptr(x) if keep_f32 else None, stream_ptr()), "relu_rows")
        return y

    def _pool(self, kind, x, B, h, w, C, dst, y_bf16, ld, keep):
        guard(x, keep)
        check(_L().sfron_pool3(ptr(x), 0, C, B, h, w, C, kind, dst, int(y_bf16), ld, stream_ptr()), "pool3")

    def _tap(self, xf, B, hw, C, out, lo):
        guard(xf)
        check(_L().sfron_global_avgpool(ptr(xf), 0, C, B, hw, C, out[C].data_ptr() + 4 * lo * C, stream_ptr()), "global_avgpool")

    def _chunk(self, images, lo, hi, out, upto):
        L, B = _L(), hi - lo
        src = images[lo:hi]
        H, W = images.shape[1], images.shape[2]
        h = w = SIZE
        xb = self._buf("bf_in", B * h * w * C_PAD, torch.bfloat16)
        guard(src, xb)
        check(L.sfron_resize_tf1_u8(ptr(src), B, H, W, h, w, C_PAD, ptr(xb), stream_ptr()), "resize_tf1_u8")
        xf, C, cur = None, C_PAD, 0
        for st in self.stem:
            if st[0] == "conv":
                _, _, cout, kh, kw, s, ph, pw = self.convs[st[1]]
                xf = self._buf(f"f_x{cur}", B * _out_size(h, kh, s, ph) * _out_size(w, kw, s, pw) * cout, torch.float32)
                h, w = self._conv(st[1], xb, B, h, w, ptr(xf), cout, xf)
                C = cout
                xb = self._relu(xf, B * h * w, C, f"bf_x{cur}", True)
                cur = 1 - cur
            elif st[0] == "max2":
                ho, wo = _out_size(h, 3, 2, 0), _out_size(w, 3, 2, 0)
                y = self._buf(f"f_x{cur}", B * ho * wo * C, torch.float32)
                self._pool(_lib.POOL_MAX_S2, xf, B, h, w, C, ptr(y), False, C, y)
                xf, h, w = y, ho, wo
                xb = self._relu(xf, B * h * w, C, f"bf_x{cur}")        # values are >= 0 already: the bf16 cast alone
                cur = 1 - cur
            else:
                if st[1] in out:
                    self._tap(xf, B, h * w, C, out, lo)
                if st[1] >= upto:
                    return
        for name, cin, width, branches in self.blocks:
            ho, wo = (_out_size(h, 3, 2, 0), _out_size(w, 3, 2, 0)) if branches[-1][0][0] == "max2" else (h, w)
            cat = self._buf(f"f_x{cur}", B * ho * wo * width, torch.float32)
            col = 0
            for br in branches:
                t, th, tw, tc = xb, h, w, cin
                for k, st in enumerate(br):
                    last = k == len(br) - 1
                    if st[0] == "conv":
                        cout = self.convs[st[1]][2]
                        if last:
                            self._conv(st[1], t, B, th, tw, cat.data_ptr() + 4 * col, width, cat)
                            col += cout
                        else:
                            _, _, _, kh, kw, s, ph, pw = self.convs[st[1]]
                            o = self._buf("f_t", B * _out_size(th, kh, s, ph) * _out_size(tw, kw, s, pw) * cout, torch.float32)
                            th, tw = self._conv(st[1], t, B, th, tw, ptr(o), cout, o)
                            t, tc = self._relu(o, B * th * tw, cout, f"bf_t{k % 2}"), cout
                    elif st[0] == "fork":
                        for i in st[1:]:
                            self._conv(i, t, B, th, tw, cat.data_ptr() + 4 * col, width, cat)
                            col += self.convs[i][2]
                    elif st[0] == "max2":
                        self._pool(_lib.POOL_MAX_S2, xf, B, h, w, cin, cat.data_ptr() + 4 * col, False, width, cat)
                        col += cin
                    else:                              # the 3x3 stride-1 pools read the fp32 row, not its bf16 copy
                        t = self._buf("bf_pool", B * h * w * cin, torch.bfloat16)
                        self._pool(_lib.POOL_AVG_S1 if st[0] == "avg" else _lib.POOL_MAX_S1, xf, B, h, w, cin, ptr(t), True, cin, t)
            assert col == width, (name, col, width)
            xf, h, w, C = cat, ho, wo, width
            xb = self._relu(xf, B * h * w, C, f"bf_x{cur}", True)
            cur = 1 - cur
            if name == "Mixed_6e":
                if 768 in out:
                    self._tap(xf, B, h * w, C, out, lo)
                if upto <= 768:
                    return
        self._tap(xf, B, h * w, C, out, lo)

    @torch.no_grad()
    def forward_u8(self, images_u8_nhwc, taps=TAPS):
        x = images_u8_nhwc
        if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3 or x.shape[0] < 1:
            raise ValueError(f"forward_u8 takes uint8 [B, H, W, 3], got {x.dtype} {tuple(x.shape)}")
        taps = tuple(int(t) for t in taps)
        if not taps or any(t not in TAPS for t in taps):
            raise ValueError(f"feature taps are {TAPS}, got {taps}")
        if self._loaded is None:
            raise _lib.SfronError("InceptionV3: load_state_dict first")
        x = x.to(self.dev).contiguous()
        B, H, W = x.shape[:3]
        out = {t: torch.empty(B, t, dtype=torch.float32, device=self.dev) for t in taps}
        n = self.chunk_size(H, W)
        for lo in range(0, B, n):
            self._chunk(x, lo, min(B, lo + n), out, max(taps))
        return out

    __call__ = forward_u8

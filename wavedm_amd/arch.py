"""HFRM -- drop-in for the reference's `models/arch.py:206-253` (the high-frequency refinement module that
`utils/restoration.py:94` runs once per image before the diffusion sampler) whose forward runs on
libwavedm_hip.so.

* same constructor signature and defaults as the reference class, same `state_dict()` keys / shapes / order
  (448 tensors, 15.94 M parameters at the `ddm_wavelet.py:139` configuration), so `lastest.pth` loads with
  `load_state_dict(strict=True)`;
* `forward(x)`: x (B, 3, H, W) fp32 NCHW on the GPU, H and W multiples of 16 -> (B, 3, H, W) fp32 NCHW;
* `convert(base_size, train_size)`: the reference's test-time local converter (`Local_Base.convert`, arch.py:114-130, which the reference
  ships and never calls): every ChannelAttn pools over a sliding window of `base_size` (at full resolution) instead of the whole map.

The parameter tree comes from the library's own table (wdm_hfrm_param_info)."""
from __future__ import annotations

import ctypes as C
import math

import torch
import torch.nn as nn

from . import _lib
from .unet import _Node, resolve_dtype


class HFRM(nn.Module):
    # batch chunk: a call of several images stays within the conv kernel's 4 GB launch range; a single image beyond it runs its GEMMs in row chunks
    MAX_PIXELS = 1 << 22
    # per image: the bound up to which every index of the path is checked; below it memory decides
    MAX_IMAGE_PIXELS = 1 << 27

    def __init__(self, in_channel=3, dim=32, mid_blk_num=1, enc_blk_nums=[], dec_blk_nums=[], win_size=8, dtype=None):
        super().__init__()
        if len(enc_blk_nums) != len(dec_blk_nums) or not 1 <= len(enc_blk_nums) <= 8:
            raise ValueError("HFRM: enc_blk_nums and dec_blk_nums must have the same length (1..8)")
        self.in_channel, self.dim = int(in_channel), int(dim)
        self.padder_size = 2 ** len(enc_blk_nums)
        self._dtype_code = resolve_dtype(None, dtype)
        if self._dtype_code in (_lib.WDM_F32X3, _lib.WDM_F16):      # the HFRM has two modes; the parity modes of the UNet (f32x3, f16) map to its exact one
            self._dtype_code = _lib.WDM_F32
        cfg = _lib.HFRMConfig()
        cfg.in_channel, cfg.dim, cfg.mid_blk_num = self.in_channel, self.dim, int(mid_blk_num)
        cfg.n_enc, cfg.n_dec = len(enc_blk_nums), len(dec_blk_nums)
        for i, v in enumerate(enc_blk_nums):
            cfg.enc_blk_nums[i] = int(v)
        for i, v in enumerate(dec_blk_nums):
            cfg.dec_blk_nums[i] = int(v)
        cfg.dtype = self._dtype_code
        self._cfg = cfg
        L = _lib.lib()
        m = C.c_void_p()
        _lib.check(L.wdm_hfrm_create(None, C.byref(cfg), C.byref(m)))
        self._m = m
        self._names = []
        name, ndim, shape = C.c_char_p(), C.c_int(), (C.c_int64 * 4)()
        for i in range(L.wdm_hfrm_num_params(m)):
            _lib.check(L.wdm_hfrm_param_info(m, i, C.byref(name), C.byref(ndim), C.byref(shape)))
            key = name.value.decode()
            self._names.append(key)
            self._register(key, tuple(int(shape[k]) for k in range(ndim.value)))
        self._packed = None
        self._packed_sig = None
        self._ws = {}
        self._local = None          # ((base_h, base_w), (train_h, train_w)) after convert(), None: global pooling
        self._max_launch = 0        # wdm_hfrm_set_max_launch_bytes; 0: the kernels' own limits

    # ---- test-time local converter (arch.py:46-130) ---------------------------------------------
    @staticmethod
    def local_sizes(base_size, train_size):
        """(base_h, base_w, train_h, train_w) of a convert() call: `base_size` an int or a pair, `train_size` (1, C, H, W) as in the reference."""
        if isinstance(base_size, int):
            base_size = (base_size, base_size)
        base_size, train_size = tuple(int(v) for v in base_size), tuple(int(v) for v in train_size)
        if len(base_size) != 2 or len(train_size) < 2:
            raise ValueError("HFRM.convert: base_size is an int or (h, w), train_size is (1, C, H, W)")
        return base_size[0], base_size[1], train_size[-2], train_size[-1]

    def convert(self, base_size=None, train_size=None, fast_imp=False):
        """`Local_Base.convert(base_size, train_size=..., fast_imp=False)`: from now on every ChannelAttn pools over a window -- at level l
        of `(train_h >> l) * base_h // train_h` rows and likewise columns, what the reference's converting forward at `train_size` freezes --
        wherever that window does not cover the map, with replicate padding at the borders; a covered map is pooled globally, bit for bit as
        before.  `convert(None)` returns to global pooling.  Test-time only: the trainer (hfrm_training) never pools locally.  Returns self."""
        if fast_imp:
            raise NotImplementedError("HFRM.convert: fast_imp=True is not implemented (the reference calls that path non-equivalent)")
        L = _lib.lib()
        if base_size is None:
            _lib.check(L.wdm_hfrm_set_local(self._m, 0, 0, 0, 0))
            self._local = None
        else:
            if train_size is None:
                raise ValueError("HFRM.convert: train_size=(1, C, H, W) is required with a base_size")
            bh, bw, th, tw = self.local_sizes(base_size, train_size)
            _lib.check(L.wdm_hfrm_set_local(self._m, bh, bw, th, tw))
            self._local = ((bh, bw), (th, tw))
        self._ws = {}
        return self

    @property
    def max_launch_bytes(self):
        """The limit on the bytes one conv-kernel launch may address, 0 (default): the kernels' own (4 GB of 32-bit buffer offsets).  A GEMM with an
        operand beyond it runs in row chunks, bit-identical to one launch; `conv_out` beyond it runs on its direct kernel.  Setting it only ever
        lowers the limit (tests, diagnosis); a value below one 256-row tile of the widest layer is refused.  Resets the cached workspace."""
        return self._max_launch

    @max_launch_bytes.setter
    def max_launch_bytes(self, nbytes):
        nbytes = int(nbytes)
        _lib.check(_lib.lib().wdm_hfrm_set_max_launch_bytes(self._m, nbytes))
        self._max_launch = nbytes
        self._ws = {}

    def chunk_rows(self, M, cin, cout, has_res=False):
        """Rows per launch of a GEMM of M rows, cin -> cout channels, under the current limit (M: one launch).  Host only."""
        rows = C.c_int64()
        _lib.check(_lib.lib().wdm_hfrm_chunk_rows(self._m, int(M), int(cin), int(cout), int(bool(has_res)), C.byref(rows)))
        return int(rows.value)

    @property
    def local_kernels(self):
        """[(kh, kw)] of the pools at level 0 .. len(enc_blk_nums) (the last is mid_blks) after convert(); [] while pooling globally."""
        if self._local is None:
            return []
        L, out = _lib.lib(), []
        kh, kw = C.c_int(), C.c_int()
        for lv in range(self._cfg.n_enc + 1):
            _lib.check(L.wdm_hfrm_local_kernel(self._m, lv, C.byref(kh), C.byref(kw)))
            out.append((kh.value, kw.value))
        return out

    def _register(self, key, shape):
        parts = key.split(".")
        node = self
        for comp in parts[:-1]:
            if comp not in node._modules:
                node.add_module(comp, _Node())
            node = node._modules[comp]
        p = torch.empty(shape, dtype=torch.float32)
        leaf = parts[-1]
        if leaf in ("beta", "gamma"):          # arch.py:165-166: zeros
            p.zero_()
        elif len(shape) > 1:
            nn.init.kaiming_uniform_(p, a=math.sqrt(5))
        elif leaf == "weight":
            p.fill_(1.0)
        else:
            p.zero_()
        node.register_parameter(leaf, nn.Parameter(p))

    def __del__(self):
        try:
            if getattr(self, "_m", None):
                _lib.lib().wdm_hfrm_destroy(self._m)
                self._m = None
        except Exception:
            pass

    def _signature(self):
        return tuple((p.data_ptr(), p._version) for p in self.parameters())

    def pack_weights(self, force=False):
        sig = self._signature()
        if not force and self._packed is not None and sig == self._packed_sig:
            return self._packed
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("HFRM: move the module to the GPU first (.to('cuda')); there is no CPU path")
        L = _lib.lib()
        with torch.cuda.device(dev):
            if self._packed is None or self._packed.device != dev:
                self._packed = torch.empty(int(L.wdm_hfrm_packed_bytes(self._m)) + 256, dtype=torch.uint8, device=dev)
                _lib.check(L.wdm_hfrm_set_packed(self._m, _lib.ptr(self._packed), self._packed.numel()))
            sd = dict(self.named_parameters())
            for key in self._names:
                src = sd[key].detach().contiguous()
                _lib.check(L.wdm_hfrm_load_param(self._m, key.encode(), _lib.ptr(src), src.numel(), _lib.stream_ptr()))
            _lib.check(L.wdm_hfrm_finalize(self._m, _lib.stream_ptr()))
        self._packed_sig = sig
        return self._packed

    def _workspace(self, B, H, W, device, keep_transposed=False):
        """The cached workspace of a (B, H, W) call.  One entry; with keep_transposed (forward_self_ensemble's members alternate between H x W and W x H) the
        entry of (B, W, H) stays beside it, so that no member allocates once both exist."""
        key = (B, H, W, str(device), self._local)
        if key not in self._ws:
            n = int(_lib.lib().wdm_hfrm_workspace_bytes(self._m, B, H, W))
            if n == 0:
                raise RuntimeError("wdm_hfrm_workspace_bytes failed: " + _lib.lib().wdm_last_error().decode())
            other = (B, W, H) + key[3:]
            kept = {other: self._ws[other]} if keep_transposed and other in self._ws else {}
            self._ws = kept                                            # everything else is released before the new one is asked for
            self._ws[key] = torch.empty(n + 256, dtype=torch.uint8, device=device)
        return self._ws[key]

    STAGES = {"block": 0, "down": 1, "up": 2, "conv_in": 3, "conv_out": 4}

    def stage_forward(self, kind, index, x, skip=None):
        """One stage on its own (wdm_hfrm_stage_forward, for unit tests): the code forward() runs, on the caller's tensors.  kind: "block" (index: the block's
        position in registration order -- encoders, decoders, mid_blks), "down" / "up" (downs[index] / ups[index] with `skip`), "conv_in", "conv_out" (the MFMA
        form; `skip` is the residual image).  x, skip: fp32 NCHW on the GPU, stored here in the model dtype as NHWC (conv_in's image stays fp32 NCHW) -> fp32
        NCHW on the GPU, exactly the values the stage stored."""
        code = self.STAGES[kind]
        x = _lib.require_cuda_f32(x, "HFRM stage input")
        self.pack_weights()
        dt = torch.bfloat16 if self._dtype_code == _lib.WDM_BF16 else torch.float32
        nhwc = lambda t: t.permute(0, 2, 3, 1).to(dt).contiguous()
        B, Cc, H, W = x.shape
        xd = x.contiguous() if kind == "conv_in" else nhwc(x)
        sk = None if skip is None else nhwc(_lib.require_cuda_f32(skip, "HFRM stage skip"))
        shape = {"block": (B, H, W, Cc), "down": (B, H // 2, W // 2, 2 * Cc), "up": (B, 2 * H, 2 * W, Cc // 2), "conv_in": (B, H, W, self.dim)}.get(kind)
        y = torch.empty(shape, dtype=dt, device=x.device) if shape else torch.empty(B, self.in_channel, H, W, dtype=torch.float32, device=x.device)
        L = _lib.lib()
        with torch.cuda.device(x.device):
            n = int(L.wdm_hfrm_stage_workspace_bytes(self._m, code, int(index), B, H, W))
            if n == 0:
                raise RuntimeError("wdm_hfrm_stage_workspace_bytes failed: " + L.wdm_last_error().decode())
            ws = torch.empty(n + 256, dtype=torch.uint8, device=x.device)
            _lib.check(L.wdm_hfrm_stage_forward(self._m, code, int(index), _lib.ptr(xd), _lib.ptr(sk) if sk is not None else None, B, H, W, _lib.ptr(y),
                                                _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
        return y if kind == "conv_out" else y.permute(0, 3, 1, 2).float().contiguous()

    def forward(self, x):
        return self._forward(x)

    def forward_self_ensemble(self, x, mode, return_members=False):
        """Geometric self-ensemble at test time: the mean of the network's outputs over the orientations of `mode` -- "none", "hflip", "flips" or "d4",
        device_data.AUGMENT_MASKS -- each output turned back.  Orientation o in 0 .. 7 is O_o(t) = o & 1: t.flip(-1), then o & 2: t.flip(-2), then o & 4:
        t.transpose(-1, -2); its inverse D_o takes the steps back in reverse order.  The members are the codes o with o & ~mask == 0, ascending (K = 1, 2, 4, 8):

            y_k = forward(O_{o_k}(x))                                    -- the bits forward returns for the host-oriented, contiguous batch
            r   = (((D y_0 + D y_1) + ...) + D y_{K-1}) * (1 / K)       -- fp32, every sum rounded once, in this order; the product is exact

        x (B, 3, H, W) fp32 on the GPU, H and W multiples of 16 (a transposed picture is W x H: legal).  "none" is forward(x): the same launches.  One member's
        output is alive at a time; with return_members=True -> (r, [y_k]) (tests, diagnosis).  Test-time only: the trainer never calls it."""
        from .device_data import augment_mask
        mask = augment_mask(mode)
        if mask == 0:
            y = self.forward(x)
            return (y, [y]) if return_members else y
        x = _lib.require_cuda_f32(x, "HFRM input")
        B, Cc, H, W = x.shape
        codes = [o for o in range(8) if o & ~mask == 0]
        L, h = _lib.lib(), _lib.handle(x.device.index or 0)
        members, acc = [], None
        with torch.cuda.device(x.device):
            xo = torch.empty(x.numel(), dtype=torch.float32, device=x.device)
            for k, o in enumerate(codes):
                if o == 0:                                                  # O_0 and D_0 are the identity: the member reads x itself
                    y = self._forward(x, keep_transposed=True)
                else:
                    xk = xo.view(B, Cc, W, H) if o & 4 else xo.view(B, Cc, H, W)
                    _lib.check(L.wdm_image_orient(h, _lib.ptr(x), B, Cc, H, W, o, _lib.ptr(xk), _lib.stream_ptr()))
                    y = self._forward(xk, keep_transposed=True)
                if return_members:
                    members.append(y)
                if o == 0 and not return_members:
                    acc = y                                                 # ... and its output is the accumulator's first value as it stands
                    continue
                if acc is None:
                    acc = torch.empty_like(x)
                scale = 1.0 / len(codes) if k == len(codes) - 1 else 1.0
                _lib.check(L.wdm_image_deorient_accumulate(h, _lib.ptr(y), B, Cc, H, W, o, int(k == 0), scale, _lib.ptr(acc), _lib.stream_ptr()))
        return (acc, members) if return_members else acc

    def _forward(self, x, keep_transposed=False):
        x = _lib.require_cuda_f32(x, "HFRM input")
        B, Cc, H, W = x.shape
        if Cc != self.in_channel:
            raise ValueError(f"HFRM: {Cc} input channels, expected {self.in_channel}")
        if H * W > self.MAX_IMAGE_PIXELS:           # before anything is launched (the library refuses the same, wdm_hfrm_forward)
            raise ValueError(f"HFRM: {H} x {W} = {H * W} pixels per image exceed the bound of 2^27 = {self.MAX_IMAGE_PIXELS}")
        self.pack_weights()
        y = torch.empty_like(x)
        chunk = max(1, self.MAX_PIXELS // (H * W))
        L = _lib.lib()
        with torch.cuda.device(x.device):
            for b0 in range(0, B, chunk):
                nb = min(chunk, B - b0)
                ws = self._workspace(nb, H, W, x.device, keep_transposed)
                _lib.check(L.wdm_hfrm_forward(self._m, _lib.ptr(x[b0:b0 + nb]), nb, H, W, _lib.ptr(y[b0:b0 + nb]),
                                              _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
        return y

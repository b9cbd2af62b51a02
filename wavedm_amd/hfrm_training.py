"""Training of the HFRM on the HIP library -- stage 1 of the reference's recipe (`train_hfrm.py`), whose `lastest.pth` stage 2 and
`restore()` load (models/ddm_wavelet.py:142-147).

`HFRMTrainer()` owns four flat fp32 device buffers -- parameters, gradients, Adam m / v -- in the layout the library reports
(`wdm_hfrm_trainer_param_info`), and runs the body of the reference's loop (train_hfrm.py:240-268):

    loss = trainer.loss_and_grads(inp, gt)      # HFRM forward, 2 * mean|255 out - 255 gt| and its backward (csrc/hfrm_train.hip)
    trainer.optimizer_step()                    # torch.optim.Adam(betas=(0.5, 0.999)), lr = 2e-4 * 0.5 ** (step / 1e5), no EMA

`state_dict()` uses the reference's keys, shapes and order; `save(path)` writes the plain state_dict that `wavedm_amd.HFRM` and the
reference's `DenoisingDiffusion_Wavelet` load with strict=True.

Two precisions: exact fp32 (the default) and `dtype="bf16-mixed"` -- activations and activation gradients stored in bf16, GEMMs on the
bf16 MFMA path with fp32 accumulation, the four flat buffers (and so every checkpoint) unchanged fp32.  `sample_sheet` builds the
reference's `sample_images` sheet [input | prediction | target] on the device."""
from __future__ import annotations

import ctypes as C
import math
from collections import OrderedDict

import torch

from . import _lib

HFRM_DEFAULTS = dict(in_channel=3, dim=32, mid_blk_num=6, enc_blk_nums=(2, 2, 2, 4), dec_blk_nums=(2, 2, 2, 2))     # train_hfrm.py:88-95


def hfrm_lr(step: int, base: float = 2e-4) -> float:
    """The learning rate train_hfrm.py:244-246 sets before optimizer step `step` (counted from 1): base * 0.5 ** (step / 100000)."""
    return base * 0.5 ** (step / 100000)


def batch_psnr(target, pred):
    """BatchPSNR (train_hfrm.py:27-31): per image, clamp both to [0, 1], RMSE over (C, H, W), 20 log10(1 / rmse)."""
    d = pred.clamp(0, 1) - target.clamp(0, 1)
    rmse = (d * d).mean(dim=(1, 2, 3)).sqrt()
    return 20 * torch.log10(1 / rmse)


MIXED = "bf16-mixed"      # a name of this module alone (not in _lib.DTYPES): no other class learns it


def _resolve_train_dtype(dtype):
    """The activation storage type of a training step: WDM_BF16 for "bf16-mixed", WDM_F32 for everything else that is accepted."""
    name = dtype or "f32"
    if name == MIXED:
        return _lib.WDM_BF16
    if name not in _lib.DTYPES:
        raise ValueError(f"unknown compute dtype {name!r} (use 'f32' or 'bf16-mixed'; 'f32x3' and 'f16' train in exact fp32 as well)")
    if _lib.DTYPES[name] == _lib.WDM_BF16:
        raise NotImplementedError("HFRMTrainer: true bf16 training (bf16 parameters and optimizer state) is not built; "
                                  "dtype='bf16-mixed' trains with bf16 activations over fp32 master state, dtype='f32' in exact fp32")
    return _lib.WDM_F32


def sample_sheet(inp, out, gt):
    """The reference's sample_images sheet (train_hfrm.py:199-220) of batch element 0: an (H, 3W, 3) uint8 tensor [input | prediction |
    target], values x * 255 in fp32 -- the prediction clamped to [0, 255] first -- truncated toward zero as the reference's .int() does
    (not the rounding of wdm_to_u8_hwc).  Computed where the tensors live."""
    a = inp[0].detach().float() * 255
    p = torch.clamp(out[0].detach().float() * 255, 0, 255)
    t = gt[0].detach().float() * 255
    sheet = torch.cat([a, p, t], dim=2).permute(1, 2, 0)
    return sheet.to(torch.int32).to(torch.uint8).contiguous()


def reference_init_state_dict(shapes, seed: int = 0):
    """The state the reference trains from (train_hfrm.py:111, `generator.apply(weights_init_normal)`, models/model_dense.py:157-168) for
    an ordered {key: shape} table:
      * every Conv weight zero, then `eye_` on its centre tap [:, :, k // 2, k // 2] -- for the depthwise conv2 that tap is a (2d, 1)
        matrix, so only [0, 0] becomes 1;
      * conv biases keep torch's default init, U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)), drawn here in table order from
        torch.Generator().manual_seed(seed);
      * LayerNorm2d weight / bias ones / zeros; beta / gamma zeros (arch.py:165-166).
    At this point every ResidualBlock is the identity."""
    g = torch.Generator().manual_seed(int(seed))
    sd = OrderedDict()
    for key, shape in shapes.items():
        shape = tuple(int(v) for v in shape)
        leaf = key.rsplit(".", 1)[-1]
        owner = key[: -len(leaf) - 1]
        if leaf in ("beta", "gamma"):
            t = torch.zeros(shape)
        elif ".norm" in "." + owner.rsplit(".", 1)[-1] and len(shape) == 1:
            t = torch.ones(shape) if leaf == "weight" else torch.zeros(shape)
        elif len(shape) == 4:
            t = torch.zeros(shape)
            k = shape[2] // 2
            n = min(shape[0], shape[1])
            t[torch.arange(n), torch.arange(n), k, k] = 1.0
        else:                                                   # a conv bias: the weight sits right before it in the table
            wshape = shapes[owner + ".weight"]
            fan_in = int(wshape[1]) * int(wshape[2]) * int(wshape[3])
            bound = 1.0 / math.sqrt(fan_in)
            t = torch.empty(shape).uniform_(-bound, bound, generator=g)
        sd[key] = t
    return sd


class HFRMTrainer:
    def __init__(self, in_channel=3, dim=32, mid_blk_num=6, enc_blk_nums=(2, 2, 2, 4), dec_blk_nums=(2, 2, 2, 2), device=None, dtype=None,
                 lr=2e-4, betas=(0.5, 0.999), eps=1e-8, grad_clip=None, skip_nonfinite=None):
        from .training import grad_guard_settings
        self.grad_clip, self.skip_nonfinite = grad_guard_settings(None, grad_clip, skip_nonfinite)      # off unless asked for (Trainer's pair; no config here)
        self._act_code = _resolve_train_dtype(dtype)
        self._dtype_code = _lib.WDM_F32                 # parameters and optimizer state: fp32 in both precisions
        if len(enc_blk_nums) != len(dec_blk_nums):
            raise ValueError("HFRMTrainer: enc_blk_nums and dec_blk_nums must have the same length")
        self.device = torch.device(device if device is not None else "cuda:0")
        if self.device.type != "cuda":
            raise RuntimeError("wavedm_amd.HFRMTrainer runs on MI355X only (no CPU path)")
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.hfrm_args = dict(in_channel=int(in_channel), dim=int(dim), mid_blk_num=int(mid_blk_num), enc_blk_nums=list(enc_blk_nums),
                              dec_blk_nums=list(dec_blk_nums))
        cfg = _lib.HFRMConfig()
        cfg.in_channel, cfg.dim, cfg.mid_blk_num = int(in_channel), int(dim), int(mid_blk_num)
        cfg.n_enc, cfg.n_dec = len(enc_blk_nums), len(dec_blk_nums)
        for i, v in enumerate(enc_blk_nums):
            cfg.enc_blk_nums[i] = int(v)
        for i, v in enumerate(dec_blk_nums):
            cfg.dec_blk_nums[i] = int(v)
        cfg.dtype = self._dtype_code
        self._cfg = cfg
        L = _lib.lib()
        t = C.c_void_p()
        _lib.check(L.wdm_hfrm_trainer_create(None, C.byref(cfg), C.byref(t)))
        self._t = t
        _lib.check(L.wdm_hfrm_trainer_set_precision(t, self._act_code))
        self.layout = OrderedDict()                     # name -> (offset, shape)
        name, ndim, shape, off = C.c_char_p(), C.c_int(), (C.c_int64 * 4)(), C.c_int64()
        for i in range(L.wdm_hfrm_trainer_num_params(t)):
            _lib.check(L.wdm_hfrm_trainer_param_info(t, i, C.byref(name), C.byref(ndim), C.byref(shape), C.byref(off)))
            self.layout[name.value.decode()] = (int(off.value), tuple(int(shape[k]) for k in range(ndim.value)))
        n = int(L.wdm_hfrm_trainer_num_floats(t))
        with torch.cuda.device(self.device):
            self.params = torch.zeros(n, device=self.device)
            self.grads = torch.zeros(n, device=self.device)
            self.exp_avg = torch.zeros(n, device=self.device)
            self.exp_avg_sq = torch.zeros(n, device=self.device)
            self._loss = torch.zeros(1, device=self.device)
            from .training import GradGuard
            self._guard = GradGuard(self.grads, self.grad_clip, self.skip_nonfinite) if (self.grad_clip > 0.0 or self.skip_nonfinite) else None
        _lib.check(L.wdm_hfrm_trainer_set_buffers(t, _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq)))
        self.step = 0
        self._ws = None
        self._ws_key = None

    def __del__(self):
        try:
            if getattr(self, "_t", None):
                _lib.lib().wdm_hfrm_trainer_destroy(self._t)
                self._t = None
        except Exception:
            pass

    # ---- parameters in the reference's naming ----------------------------------------------------------------------
    def _view(self, flat, name):
        off, shape = self.layout[name]
        return flat[off:off + math.prod(shape)].view(shape)

    def param_shapes(self):
        return OrderedDict((k, v[1]) for k, v in self.layout.items())

    def state_dict(self):
        return OrderedDict((k, self._view(self.params, k).clone()) for k in self.layout)

    def grad_dict(self):
        return OrderedDict((k, self._view(self.grads, k).clone()) for k in self.layout)

    def load_state_dict(self, sd, strict=True):
        sd = {k[len("module."):] if k.startswith("module.") else k: v for k, v in sd.items()}
        missing = [k for k in self.layout if k not in sd]
        extra = [k for k in sd if k not in self.layout]
        if strict and (missing or extra):
            raise RuntimeError(f"HFRMTrainer.load_state_dict: missing {missing[:4]}, unexpected {extra[:4]}")
        for k in self.layout:
            if k in sd:
                v = torch.as_tensor(sd[k])
                if tuple(v.shape) != self.layout[k][1]:
                    raise RuntimeError(f"HFRMTrainer.load_state_dict: {k} has shape {tuple(v.shape)}, expected {self.layout[k][1]}")
                self._view(self.params, k).copy_(v.to(self.device, torch.float32))

    def init_reference(self, seed: int = 0):
        """weights_init_normal (train_hfrm.py:111) with torch-default conv biases from a seeded generator: see reference_init_state_dict."""
        self.load_state_dict(reference_init_state_dict(self.param_shapes(), seed), strict=True)

    def save(self, path):
        """The plain state_dict (train_hfrm.py:303-305 saves generator.module.state_dict(): no `module.` prefix, no optimizer state)."""
        torch.save(OrderedDict((k, v.cpu()) for k, v in self.state_dict().items()), path)

    # ---- precision ---------------------------------------------------------------------------------------------------
    @property
    def precision(self):
        return MIXED if self._act_code == _lib.WDM_BF16 else "f32"

    def set_precision(self, dtype):
        """Switch between "f32" and "bf16-mixed" between steps; parameters, moments and the step count stay."""
        code = _resolve_train_dtype(dtype)
        _lib.check(_lib.lib().wdm_hfrm_trainer_set_precision(self._t, code))
        self._act_code = code

    # ---- one step ----------------------------------------------------------------------------------------------------
    def _workspace(self, B, H, W):
        key = (B, H, W, self._act_code)
        if self._ws_key != key:
            n = int(_lib.lib().wdm_hfrm_trainer_workspace_bytes(self._t, B, H, W))
            if n == 0:
                raise RuntimeError("wdm_hfrm_trainer_workspace_bytes failed: " + _lib.lib().wdm_last_error().decode(errors="replace"))
            self._ws = None
            self._ws = torch.empty(n + 256, dtype=torch.uint8, device=self.device)
            self._ws_key = key
        return self._ws

    def _step(self, inp, gt, dy, out):
        inp = _lib.require_cuda_f32(inp, "HFRM input")
        B, Cc, H, W = inp.shape
        if Cc != self.hfrm_args["in_channel"]:
            raise ValueError(f"HFRMTrainer: {Cc} input channels, expected {self.hfrm_args['in_channel']}")
        with torch.cuda.device(self.device):
            ws = self._workspace(B, H, W)
            _lib.check(_lib.lib().wdm_hfrm_trainer_step(self._t, _lib.ptr(inp), _lib.ptr(gt) if gt is not None else None, _lib.ptr(dy) if dy is not None else None,
                                                        B, H, W, _lib.ptr(self._loss), _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))

    def loss_and_grads(self, inp, gt, return_output=False):
        """inp, gt (B, 3, H, W) in [0, 1], H and W multiples of 16.  Fills self.grads with the gradient of 2 * mean|255 out - 255 gt|;
        returns that loss as a 0-dim device tensor (and the network output when asked)."""
        gt = _lib.require_cuda_f32(gt, "HFRM target")
        out = torch.empty_like(gt)
        if tuple(gt.shape) != tuple(inp.shape):
            raise ValueError("HFRMTrainer: input and target shapes differ")
        self._step(inp, gt, None, out)
        return (self._loss[0], out) if return_output else self._loss[0]

    def backward_from(self, inp, dy):
        """Back-propagate an arbitrary upstream gradient dy (B, 3, H, W) of the output: fills self.grads, returns the output."""
        dy = _lib.require_cuda_f32(dy, "dy")
        if tuple(dy.shape) != tuple(inp.shape):
            raise ValueError("HFRMTrainer: dy must have the input's shape")
        out = torch.empty_like(dy)
        self._step(inp, None, dy, out)
        return out

    STAGES = {"block": 0, "down": 1, "up": 2, "conv_in": 3, "conv_out": 4}

    def stage(self, kind, index, x, dy, skip=None, dres=None):
        """One stage's forward and backward on their own (wdm_hfrm_trainer_stage, for unit tests): the members a step runs, on the caller's tensors, in the
        current precision.  kind / index as HFRM.stage_forward.  x, dy, skip, dres: fp32 NCHW on the GPU, stored here in the activation type as NHWC (conv_in's
        image, conv_out's image `skip` and its dy stay fp32 NCHW); dres (kind "down" only): the gradient that arrived over the skip connection, zero when absent.
        -> (y, dx) fp32 NCHW, exactly the values the stage stored (dx is None for conv_in); the stage's entries of self.grads are written, no others."""
        code = self.STAGES[kind]
        x = _lib.require_cuda_f32(x, "HFRM stage input")
        dy = _lib.require_cuda_f32(dy, "HFRM stage dy")
        dt = torch.bfloat16 if self._act_code == _lib.WDM_BF16 else torch.float32
        nhwc = lambda t: t.permute(0, 2, 3, 1).to(dt).contiguous()
        B, Cc, H, W = x.shape
        dim, nc = self.hfrm_args["dim"], self.hfrm_args["in_channel"]
        xd = x if kind == "conv_in" else nhwc(x)
        dyd = dy if kind == "conv_out" else nhwc(dy)
        sk = None
        if skip is not None:
            skip = _lib.require_cuda_f32(skip, "HFRM stage skip")
            sk = skip if kind == "conv_out" else nhwc(skip)
        shape = {"block": (B, H, W, Cc), "down": (B, H // 2, W // 2, 2 * Cc), "up": (B, 2 * H, 2 * W, Cc // 2), "conv_in": (B, H, W, dim)}.get(kind)
        y = torch.empty(shape, dtype=dt, device=x.device) if shape else torch.empty(B, nc, H, W, dtype=torch.float32, device=x.device)
        if tuple(dyd.shape) != tuple(y.shape):
            raise ValueError(f"HFRMTrainer.stage: dy has shape {tuple(dy.shape)}, the stage's output {tuple(y.shape)} (NHWC)")
        if dres is not None and kind != "down":
            raise ValueError("HFRMTrainer.stage: dres is the skip gradient of kind 'down' only")
        dx = None
        if kind != "conv_in":
            dx = nhwc(_lib.require_cuda_f32(dres, "HFRM stage dres")) if dres is not None else torch.zeros(xd.shape, dtype=dt, device=x.device)
            if tuple(dx.shape) != tuple(xd.shape):
                raise ValueError("HFRMTrainer.stage: dres must have the input's shape")
        L = _lib.lib()
        with torch.cuda.device(self.device):
            n = int(L.wdm_hfrm_trainer_stage_workspace_bytes(self._t, code, int(index), B, H, W))
            if n == 0:
                raise RuntimeError("wdm_hfrm_trainer_stage_workspace_bytes failed: " + L.wdm_last_error().decode(errors="replace"))
            ws = torch.empty(n + 256, dtype=torch.uint8, device=self.device)
            _lib.check(L.wdm_hfrm_trainer_stage(self._t, code, int(index), _lib.ptr(xd), _lib.ptr(sk) if sk is not None else None, _lib.ptr(dyd), B, H, W, _lib.ptr(y),
                                                _lib.ptr(dx) if dx is not None else None, _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
        back = lambda t: t.permute(0, 3, 1, 2).float().contiguous()
        return (y if kind == "conv_out" else back(y)), (None if dx is None else back(dx))

    def optimizer_step(self, lr=None):
        """torch.optim.Adam step number self.step + 1 (no weight decay, no EMA); lr defaults to the reference's schedule on self.lr."""
        self.step += 1
        lr = hfrm_lr(self.step, self.lr) if lr is None else float(lr)
        with torch.cuda.device(self.device):
            if self._guard is not None:      # norm of self.grads, then Adam behind the record; self.step counts calls, a skipped step included (Trainer.optimizer_step)
                self._guard.run()
                _lib.check(_lib.lib().wdm_hfrm_trainer_adam_guarded(self._t, self.step, lr, self.betas[0], self.betas[1], self.eps, 0.0, self._guard.ptr,
                                                                    _lib.stream_ptr()))
                return
            _lib.check(_lib.lib().wdm_hfrm_trainer_adam(self._t, self.step, lr, self.betas[0], self.betas[1], self.eps, 0.0, _lib.stream_ptr()))

    grad_norm = property(lambda self: self._guard.norm if self._guard is not None else None, doc="Trainer.grad_norm")
    clip_coef = property(lambda self: self._guard.coef if self._guard is not None else None, doc="Trainer.clip_coef")
    skipped_steps = property(lambda self: self._guard.skipped_steps if self._guard is not None else 0, doc="Trainer.skipped_steps")

    def train_step(self, inp, gt, return_output=False):
        """One iteration of train_hfrm.py's loop: loss, backward, Adam.  Returns (loss, per-image PSNR of this step's output), both on the device
        (and that output when asked: the sample sheet is drawn from it)."""
        loss, out = self.loss_and_grads(inp, gt, return_output=True)
        loss, psnr = loss.clone(), batch_psnr(gt, out)
        self.optimizer_step()
        return (loss, psnr, out) if return_output else (loss, psnr)

    def train_step_from_store(self, store, batch_size=8, data_seed=None, return_output=False, return_batch=False, augment=None):
        """train_step on whole images of a DeviceImageStore (device_data.py): item j of step s is global item (s - 1) * batch_size + j of the store's item stream
        (epoch permutations keyed by the data seed; no crop), gathered to float on the device by one kernel.  All images must have one size.  The seed is
        `data_seed`, else this trainer's (drawn once from torch's global generator).  return_batch appends (inp, gt).  augment ("none", "hflip", "flips", "d4";
        default none): each pair in its drawn orientation; images that are not square take no transpose (DeviceImageStore.whole_image_mask)."""
        if data_seed is not None:
            self.data_seed = int(data_seed) & ((1 << 63) - 1)
        if getattr(self, "data_seed", None) is None:
            from .device_data import draw_data_seed
            self.data_seed = draw_data_seed()
        inp, gt = store.step_images(self.data_seed, self.step + 1, int(batch_size), augment=augment)
        res = self.train_step(inp, gt, return_output=return_output)
        return res + (inp, gt) if return_batch else res

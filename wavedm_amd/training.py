"""Training step of the wavelet-domain UNet on the HIP library.

`Trainer(config)` owns flat fp32 device buffers -- parameters, gradients, EMA shadow and the state of the configured optimizer (Adam: m / v) -- in the layout the library
reports (`wdm_trainer_param_info`), and runs the body of the reference's training loop (`models/ddm_wavelet.py:259-272`):

    loss = trainer.loss_and_grads(x0, t, e)     # noise_estimation_loss (:108-124) forward + backward
    trainer.allreduce_grads()                   # what DistributedDataParallel does in the reference (:168), one RCCL all-reduce
    trainer.optimizer_step()                    # the optimizer of utils/optimize.py:5-14 + EMAHelper.update (:48-53)

`optim.optimizer` / `optim.amsgrad` select one of the four optimizers the reference's `get_optimizer` can build (`optimizer_spec`): Adam, Adam with amsgrad,
RMSProp, SGD -- torch 2.10's single-tensor update rules, each one HIP kernel over the flat buffers with the EMA update in the same pass.

`state_dict()` / `load_state_dict()` use the reference's keys and shapes, `ema_state_dict()` is `EMAHelper.state_dict()`; a checkpoint
written by `save_checkpoint` has the reference's dict format (ddm_wavelet.py:282-292) and loads in `DenoisingDiffusion_Wavelet`.

`model.dropout` (every ResnetBlock's `conv2(dropout(silu(norm2(h))))`, models/unet.py:129): the masks are drawn inside the GroupNorm kernels from a
counter-based generator (csrc/dropout.h) keyed by `dropout_seed` and counted by (element, block, optimizer step) -- they are not torch's stream, so a
run matches the reference's in distribution, not bit for bit.  `Trainer.dropout_masks` shows what the next step draws."""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict

import torch

from . import _lib, sampling
from .unet import _make_config, reference_param_order, resolve_dtype

_MASK63 = (1 << 63) - 1


def dropout_rank_seed(base: int, rank: int) -> int:
    """The dropout seed rank `rank` of a data-parallel run uses: ranks must not share masks (their samples differ, their masks must too), and every rank can
    derive its own from the one base seed the checkpoint holds.  Rank 0 keeps the base seed; rank r adds r times an odd 63-bit constant (2^63 / golden ratio):
    multiplication by an odd number is a bijection modulo 2^63, so all ranks of any world below 2^63 differ."""
    return (int(base) + int(rank) * 0x4F1BBCDCBFA53E0B) & _MASK63


# the per-parameter state tensors of each rule, in the order of the library's state slots (include/wavedm.h)
STATE_NAMES = {"adam": ("exp_avg", "exp_avg_sq"), "amsgrad": ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"), "rmsprop": ("square_avg",), "sgd": ("momentum_buffer",)}
_RULE_CODES = {"adam": _lib.WDM_OPT_ADAM, "amsgrad": _lib.WDM_OPT_AMSGRAD, "rmsprop": _lib.WDM_OPT_RMSPROP, "sgd": _lib.WDM_OPT_SGD}
_RULE_TITLES = {"adam": "Adam", "amsgrad": "Adam(amsgrad=True)", "rmsprop": "RMSprop", "sgd": "SGD"}


def optimizer_spec(config):
    """The optimizer `get_optimizer(config, parameters)` of the reference builds (utils/optimize.py:5-14), as {"rule", "lr", "betas", "eps", "weight_decay",
    "alpha", "momentum"} with rule in adam / amsgrad / rmsprop / sgd and every value what that call hands to torch.optim -- including what it does NOT hand over:
      RMSProp  optim.RMSprop(parameters, lr, weight_decay): optim.eps is ignored, eps is torch's default 1e-8 (alpha 0.99, momentum 0, not centered)
      SGD      optim.SGD(parameters, lr, momentum=0.9): optim.weight_decay is ignored, weight decay is 0 (dampening 0, no Nesterov)
    Keys a rule does not use hold torch's defaults.  A config without an `optim` section, or without some of its keys, gets the values of raindrop_wavelet.yml's
    optimizer (Adam, amsgrad False, eps 1e-8, weight decay 0) and lr 4e-5.  Needs no GPU."""
    opt = getattr(config, "optim", None)
    name = getattr(opt, "optimizer", "Adam")
    spec = {"rule": "adam", "lr": float(getattr(opt, "lr", 4e-5)), "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.0, "alpha": 0.99, "momentum": 0.0}
    if name == "Adam":
        spec.update(rule="amsgrad" if getattr(opt, "amsgrad", False) else "adam", eps=float(getattr(opt, "eps", 1e-8)),
                    weight_decay=float(getattr(opt, "weight_decay", 0.0)))
    elif name == "RMSProp":
        spec.update(rule="rmsprop", weight_decay=float(getattr(opt, "weight_decay", 0.0)))
    elif name == "SGD":
        spec.update(rule="sgd", momentum=0.9)
    else:
        raise NotImplementedError("Optimizer {} not understood.".format(name))
    return spec


def grad_guard_settings(config=None, grad_clip=None, skip_nonfinite=None):
    """(grad_clip, skip_nonfinite) of a run: the arguments where given, else `optim.grad_clip` (the maximal global 2-norm of the gradient, what the DDIM code base
    hands to clip_grad_norm_; 0 = off) and `optim.skip_nonfinite` (drop a step whose gradient holds a NaN or an infinity) of the config, else off.  Both keys are
    this package's: the reference's configs have neither and the shipped ones stay as they are.  A negative or NaN grad_clip is a ValueError.  Needs no GPU."""
    opt = getattr(config, "optim", None)
    clip = getattr(opt, "grad_clip", 0) if grad_clip is None else grad_clip
    skip = getattr(opt, "skip_nonfinite", False) if skip_nonfinite is None else skip_nonfinite
    clip = 0.0 if clip is None else float(clip)
    if clip != clip or clip < 0.0:
        raise ValueError(f"optim.grad_clip = {clip!r}: a maximal gradient norm is positive (0 switches clipping off)")
    return clip, bool(skip)


class GradGuard:
    """The guard of one flat gradient buffer on the device (include/wavedm.h: wdm_grad_guard): its record {norm, coef, skip, skipped_total} and the scratch of the
    reduction.  `run()` enqueues the two launches; nothing comes back to the host until somebody reads `skipped_steps`."""

    def __init__(self, grads, grad_clip, skip_nonfinite):
        self.grads, self.grad_clip, self.skip_nonfinite = grads, float(grad_clip), bool(skip_nonfinite)
        self.record = torch.zeros(4, dtype=torch.int32, device=grads.device)
        self._floats = self.record.view(torch.float32)
        self._scratch = torch.empty(int(_lib.lib().wdm_grad_guard_scratch_bytes()) // 8, dtype=torch.float64, device=grads.device)

    def run(self):
        dev = self.grads.device
        _lib.check(_lib.lib().wdm_grad_guard(_lib.handle(dev.index or 0), _lib.ptr(self.grads), self.grads.numel(), self.grad_clip, int(self.skip_nonfinite),
                                             _lib.ptr(self.record), _lib.ptr(self._scratch), self._scratch.numel() * 8, _lib.stream_ptr()))

    @property
    def ptr(self):
        return _lib.ptr(self.record)

    norm = property(lambda self: self._floats[0])
    coef = property(lambda self: self._floats[1])
    skipped_steps = property(lambda self: int(self.record[3].item()))


def torch_optimizer(spec, parameters, **kw):
    """The torch.optim object of an optimizer_spec over `parameters` (what the reference instantiates; the tests' yardstick)."""
    if spec["rule"] in ("adam", "amsgrad"):
        return torch.optim.Adam(parameters, lr=spec["lr"], weight_decay=spec["weight_decay"], betas=tuple(spec["betas"]), amsgrad=spec["rule"] == "amsgrad",
                                eps=spec["eps"], **kw)
    if spec["rule"] == "rmsprop":
        return torch.optim.RMSprop(parameters, lr=spec["lr"], alpha=spec["alpha"], eps=spec["eps"], weight_decay=spec["weight_decay"], **kw)
    return torch.optim.SGD(parameters, lr=spec["lr"], momentum=spec["momentum"], weight_decay=spec["weight_decay"], **kw)


def torch_optimizer_state_dict(spec, step, tensors):
    """`torch.optim.X.state_dict()` of the optimizer of `spec` after `step` steps: tensors = {state name: [one tensor per parameter, in model.parameters() order]}
    for the names of STATE_NAMES[rule].  The entries and the param_groups keys are the ones torch 2.10 writes, so X.load_state_dict accepts the result."""
    rule = spec["rule"]
    names = STATE_NAMES[rule]
    n = len(tensors[names[0]])
    state = {}
    for i in range(n):
        e = {} if rule == "sgd" else {"step": torch.tensor(float(step))}           # (SGD keeps no step count)
        for k in names:
            e[k] = tensors[k][i]
        state[i] = e
    if rule in ("adam", "amsgrad"):
        group = {"lr": spec["lr"], "betas": tuple(spec["betas"]), "eps": spec["eps"], "weight_decay": spec["weight_decay"], "amsgrad": rule == "amsgrad",
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None}
        if rule == "amsgrad":
            group["decoupled_weight_decay"] = False
    elif rule == "rmsprop":
        group = {"lr": spec["lr"], "momentum": 0.0, "alpha": spec["alpha"], "eps": spec["eps"], "centered": False, "weight_decay": spec["weight_decay"],
                 "capturable": False, "foreach": None, "maximize": False, "differentiable": False}
    else:
        group = {"lr": spec["lr"], "momentum": spec["momentum"], "dampening": 0.0, "weight_decay": spec["weight_decay"], "nesterov": False, "maximize": False,
                 "foreach": None, "differentiable": False, "fused": None}
    group["params"] = list(range(n))
    return {"state": state, "param_groups": [group]}


def _checkpoint_rule(osd):
    """Which of the four optimizers wrote a torch.optim state dict: by the hyper-parameters of its param group, else by the names of its state tensors."""
    g = osd["param_groups"][0] if osd.get("param_groups") else {}
    e = next(iter(osd["state"].values()), {}) if osd.get("state") else {}
    if "betas" in g or "exp_avg" in e:
        return "amsgrad" if (g.get("amsgrad", False) or "max_exp_avg_sq" in e) else "adam"
    if "alpha" in g or "square_avg" in e:
        return "rmsprop"
    if "nesterov" in g or "dampening" in g or "momentum_buffer" in e:
        return "sgd"
    return None


def attn_long_workspace_bytes(model, B: int, R: int, dsize: int) -> int:
    """What the AttnBlocks on maps beyond 512 tokens add to a training step's workspace (train_unet.hip: op_attn): the softmax matrix P of every such block, kept
    for the backward pass (B N^2 elements each), and at the largest of them the transients of one block -- fp32 scores S or dP, dS, and the two transposed operands.
    Blocks of up to 512 tokens are covered by the per-pixel term of the caller, as before.  Counting them here means a workspace that is too small is enlarged before
    the first launch of a step instead of by the double-and-retry path in the middle of one."""
    nlev, nrb = len(model.ch_mult), int(model.num_res_blocks)
    attn = [int(a) for a in model.attn_resolutions]
    kept, transient = 0, 0
    for lvl in range(nlev):
        res = R >> lvl
        n = res * res
        blocks = (2 * nrb + 1 if res in attn else 0) + (1 if lvl == nlev - 1 else 0)      # down + up blocks of the level; mid.attn_1 on the coarsest map
        if n <= 512 or not blocks:
            continue
        kept += blocks * B * n * n * dsize
        transient = max(transient, B * n * n * (4 + 3 * dsize))
    return kept + transient


class Trainer:
    def __init__(self, config, device=None, dtype=None, lr=None, betas=(0.9, 0.999), eps=None, weight_decay=None, ema_mu=0.9999, use_mse=None, dropout=None, dropout_seed=None,
                 grad_clip=None, skip_nonfinite=None, data_seed=None):
        self.config = config
        # the seed of the device-resident data path (train_step_from_store; device_data.py): given, restored from a checkpoint, or drawn at the first step from
        # the store -- never by a trainer that is fed tensors, which consumes the random numbers it always did
        self.data_seed = (int(data_seed) & _MASK63) if data_seed is not None else None
        self.grad_clip, self.skip_nonfinite = grad_guard_settings(config, grad_clip, skip_nonfinite)
        self.device = torch.device(device if device is not None else getattr(config, "device", "cuda:0"))
        if self.device.type != "cuda":
            raise RuntimeError("wavedm_amd.Trainer runs on MI355X only (no CPU path)")
        self._dtype_code = resolve_dtype(config, dtype)
        if self._dtype_code in (_lib.WDM_F32X3, _lib.WDM_F16):      # training has two modes: f32x3 / f16 (inference modes) train in exact fp32
            self._dtype_code = _lib.WDM_F32
        spec = optimizer_spec(config)                   # utils/optimize.py:5-14; the explicit keyword arguments override
        self.rule = spec["rule"]
        self.lr = float(lr if lr is not None else spec["lr"])
        self.eps = float(eps if eps is not None else spec["eps"])
        self.weight_decay = float(weight_decay if weight_decay is not None else spec["weight_decay"])
        self.betas, self.ema_mu = (float(betas[0]), float(betas[1])), float(ema_mu)
        self.alpha, self.momentum = float(spec["alpha"]), float(spec["momentum"])
        # model.dropout (unet.py:99, :129): masks drawn in the kernels (csrc/dropout.h); the seed is this run's, the masks depend on (seed, rank, step) alone
        self.dropout = float(dropout if dropout is not None else (getattr(getattr(config, "model", None), "dropout", 0.0) or 0.0))
        if not 0.0 <= self.dropout < 1.0:
            raise ValueError(f"model.dropout = {self.dropout!r}: must lie in [0, 1)")
        # the base seed: given, or a 63-bit draw from torch's global generator (torch.manual_seed fixes a run) -- drawn only by a trainer that uses dropout, so that
        # a run without it consumes the random numbers it always did; None until then
        self.dropout_seed = (int(dropout_seed) & _MASK63) if dropout_seed is not None else None
        self._dropout_seed_fresh = dropout_seed is None          # (restore_dropout_seed says so once when a resumed checkpoint has no seed)
        if self.dropout > 0.0:
            self._ensure_dropout_seed()
        self._dropout_armed = False                               # the library handle holds p > 0 (wdm_trainer_set_dropout)
        # training.use_mse (ddm_wavelet.py:263-266): back-propagate the x0-space loss instead of the noise-space one
        self.use_mse = bool(use_mse if use_mse is not None else getattr(getattr(config, "training", None), "use_mse", False))
        L = _lib.lib()
        self._cfg = _make_config(config, self._dtype_code)
        t = C.c_void_p()
        _lib.check(L.wdm_trainer_create(None, C.byref(self._cfg), C.byref(t)))
        self._t = t
        self.layout = OrderedDict()                     # name -> (offset, shape)
        name, ndim, shape, off = C.c_char_p(), C.c_int(), (C.c_int64 * 4)(), C.c_int64()
        for i in range(L.wdm_trainer_num_params(t)):
            _lib.check(L.wdm_trainer_param_info(t, i, C.byref(name), C.byref(ndim), C.byref(shape), C.byref(off)))
            self.layout[name.value.decode()] = (int(off.value), tuple(int(shape[k]) for k in range(ndim.value)))
        n = int(L.wdm_trainer_num_floats(t))
        self._n_floats = n
        with torch.cuda.device(self.device):
            self.params = torch.zeros(n, device=self.device)
            self.grads = torch.zeros(n, device=self.device)
            # only the state the rule needs, under torch's names: exp_avg / exp_avg_sq (/ max_exp_avg_sq), square_avg, momentum_buffer -- also attributes of the trainer
            self.opt_state = OrderedDict((k, torch.zeros(n, device=self.device)) for k in STATE_NAMES[self.rule])
            self.ema = torch.zeros(n, device=self.device)
            # the guard of the step (optim.grad_clip / optim.skip_nonfinite): only a trainer that asks for it owns a record, and only such a trainer launches
            # the reduction and the guarded update -- without it optimizer_step is the call it always was
            self._guard = GradGuard(self.grads, self.grad_clip, self.skip_nonfinite) if (self.grad_clip > 0.0 or self.skip_nonfinite) else None
        for k, buf in self.opt_state.items():
            setattr(self, k, buf)
        self._momentum_fresh = True                     # SGD: no step has filled the momentum buffer yet (torch creates it from the first gradient)
        _lib.check(L.wdm_trainer_set_objective(t, 1 if self.use_mse else 0))
        if self.rule == "adam":
            _lib.check(L.wdm_trainer_set_buffers(t, _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq), _lib.ptr(self.ema)))
        else:
            _lib.check(L.wdm_trainer_set_buffers(t, _lib.ptr(self.params), _lib.ptr(self.grads), None, None, _lib.ptr(self.ema)))
            slots = [_lib.ptr(b) for b in self.opt_state.values()] + [None] * (3 - len(self.opt_state))
            _lib.check(L.wdm_trainer_set_optimizer(t, _RULE_CODES[self.rule], *slots))
        betas_t = sampling.get_beta_schedule(beta_schedule=config.diffusion.beta_schedule, beta_start=config.diffusion.beta_start,
                                             beta_end=config.diffusion.beta_end, num_diffusion_timesteps=config.diffusion.num_diffusion_timesteps)
        self.betas_t = torch.from_numpy(betas_t).float().to(self.device)
        self.num_timesteps = int(self.betas_t.shape[0])
        self.step = 0
        self._ws = None
        m = config.model
        self._c_t0 = int(m.in_channels)                 # x0 = [x_cond (in_channels) | x_tar (pred_channels) | x_other]
        self._loss = torch.zeros(1, device=self.device)

    def __del__(self):
        try:
            if getattr(self, "_t", None):
                _lib.lib().wdm_trainer_destroy(self._t)
                self._t = None
        except Exception:
            pass

    # ---- parameters in the reference's naming ----------------------------------------------------------------------
    def _view(self, flat, name):
        off, shape = self.layout[name]
        n = 1
        for v in shape:
            n *= v
        return flat[off:off + n].view(shape)

    def state_dict(self):
        return OrderedDict((k, self._view(self.params, k).clone()) for k in self.layout)

    def ema_state_dict(self):
        return OrderedDict((k, self._view(self.ema, k).clone()) for k in self.layout)

    def grad_dict(self):
        return OrderedDict((k, self._view(self.grads, k).clone()) for k in self.layout)

    def load_state_dict(self, sd, strict=True, init_ema=True):
        sd = {k[len("module."):] if k.startswith("module.") else k: v for k, v in sd.items()}
        missing = [k for k in self.layout if k not in sd]
        extra = [k for k in sd if k not in self.layout]
        if strict and (missing or extra):
            raise RuntimeError(f"Trainer.load_state_dict: missing {missing[:4]}, unexpected {extra[:4]}")
        for k in self.layout:
            if k in sd:
                self._view(self.params, k).copy_(sd[k].to(self.device, torch.float32))
        if init_ema:
            self.ema.copy_(self.params)                 # EMAHelper.register (ddm_wavelet.py:40-46)

    # ---- one step ----------------------------------------------------------------------------------------------------
    def loss_and_grads(self, x0, t, e, return_output=False):
        """x0 (B, Cin, R, R) wavelet-domain [x_cond | x_tar | x_other] (Cin = the UNet's input width, 96 for every other_channels_begin == pred_channels setting);
        t (B,) long; e (B, pred_channels, R, R).  Fills self.grads; returns the
        loss as a 0-dim device tensor (and the network output when asked)."""
        x0 = _lib.require_cuda_f32(x0, "x0")
        e = _lib.require_cuda_f32(e, "e")
        B, Cc, R, _ = x0.shape
        t = t.to(self.device)
        a = (1 - self.betas_t).cumprod(dim=0).index_select(0, t.long())          # ddm_wavelet.py:109
        sa, s1m = a.sqrt().contiguous(), (1.0 - a).sqrt().contiguous()
        tf = t.float().contiguous()
        out = torch.empty(B, int(self.config.model.out_ch), R, R, device=self.device) if return_output else None
        with torch.cuda.device(self.device):
            # workspace = every saved activation + its gradient + operand transposes of the largest layer.  It is sized from the batch
            # (288 GB of HBM: generosity is cheap) and doubled on demand: the library reports exhaustion as an error, never overruns.
            # ... plus the forward AND dgrad weight layouts of every conv, packed at the start of the step and kept for its whole length (train_unet.hip: pack_region):
            # about twice the parameter bytes in the model dtype -- without this term small batches took the double-and-retry path on every first step
            dsize = 2 if self._dtype_code == _lib.WDM_BF16 else 4
            need = B * Cc * R * R * 4 * 160 + 2 * self._n_floats * dsize + (1 << 28) + attn_long_workspace_bytes(self.config.model, B, R, dsize)
            if self._ws is None or self._ws.numel() < need:
                self._ws = None
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            if self.dropout > 0.0 or self._dropout_armed:          # (p = 0 on a handle that holds p = 0: the step of a model without dropout, not one call more)
                _lib.check(_lib.lib().wdm_trainer_set_dropout(self._t, self.dropout, self.rank_dropout_seed(), self.step + 1))
                self._dropout_armed = self.dropout > 0.0
            for attempt in range(4):
                ws = self._ws
                rc = _lib.lib().wdm_trainer_step(self._t, _lib.ptr(x0), _lib.ptr(tf), _lib.ptr(sa), _lib.ptr(s1m), _lib.ptr(e), B, self._c_t0, _lib.ptr(self._loss),
                                                 _lib.ptr(out) if out is not None else None, _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
                if rc == _lib.WDM_ENOMEM and attempt < 3:
                    torch.cuda.synchronize(self.device)
                    n = ws.numel() * 2
                    self._ws = ws = None
                    self._ws = torch.empty(n, dtype=torch.uint8, device=self.device)
                    continue
                _lib.check(rc)
                break
        return (self._loss[0], out) if return_output else self._loss[0]

    # ---- one stage of the step on its own ------------------------------------------------------------------------------
    def stage_names(self, kind):
        """The stages of `kind` ("resblock", "attn", "conv") by state_dict prefix, in the library's index order."""
        if kind == "resblock":
            return [k[:-len(".norm2.weight")] for k in self.layout if k.endswith(".norm2.weight")]
        if kind == "attn":
            return [k[:-len(".q.weight")] for k in self.layout if k.endswith(".q.weight")]
        return [k[:-len(".weight")] for k, (_, shape) in self.layout.items() if k.endswith(".weight") and len(shape) == 4]

    def stage(self, kind, index=0, x0=None, x1=None, dy=None, temb_all=None, d_temb_all=None, t=None, e=None, sa=None, s1m=None, c_t0=None, dx0=None, dx1=None):
        """One stage's forward and backward on their own (wdm_trainer_stage, for unit tests): the members and graph ops a step chains, on the caller's tensors, with
        the weights packed from self.params as a step packs them.  kind: "resblock", "attn", "conv", "temb", "input", "head"; index: a position in stage_names(kind)
        or one of its names.  Activations (x0, x1, dy) and activation gradients (dx0, dx1) are fp32 NCHW on the GPU here and are stored as NHWC in the trainer's
        dtype for the call; dx0 / dx1 given = the gradient a later consumer already left, to which the stage adds.  temb_all / d_temb_all: (B, temb_rows) fp32 --
        a resblock reads temb_all and writes ITS rows of d_temb_all in place; "temb" reads d_temb_all.  "input": x0 the fp32 NCHW image, e, sa, s1m, c_t0; "head": x0 = h, e
        (sa, s1m under use_mse).  Dropout as a step of self.step + 1 draws it.
        -> dict of fp32 tensors: y, dx0, dx1 (NCHW, the stored values), x96 (input), temb_all (temb), out (head, NCHW), loss; the stage's entries of self.grads are written."""
        L = _lib.lib()
        code = _lib.WDM_TRAINER_STAGES[kind]
        if isinstance(index, str):
            index = self.stage_names(kind).index(index)
        dt = torch.bfloat16 if self._dtype_code == _lib.WDM_BF16 else torch.float32
        dev = self.device
        nhwc = lambda v, n: _lib.require_cuda_f32(v, n).permute(0, 2, 3, 1).to(dt).contiguous()
        back = lambda v: v.permute(0, 3, 1, 2).float().contiguous()
        f32 = lambda v, n: None if v is None else _lib.require_cuda_f32(v, n)
        io, keep, out = _lib.TrainerStageIO(), [], {}

        def put(field, v):
            if v is not None:
                keep.append(v)
                setattr(io, field, v.data_ptr())
            return v
        m = self.config.model
        if kind == "temb":
            t = put("t", f32(t.float(), "t"))
            B, H, W = int(t.shape[0]), 1, 1
            put("d_temb_all", f32(d_temb_all, "d_temb_all"))
            out["temb_all"] = put("temb_all", torch.empty_like(d_temb_all))
        else:
            B, _, H, W = x0.shape
            if kind == "input":
                put("x0", f32(x0, "x0"))
                x96 = put("x96", torch.empty(B, H, W, int(x0.shape[1]), dtype=dt, device=dev))
                io.c_t0 = int(self._c_t0 if c_t0 is None else c_t0)
            else:
                xd = put("x0", nhwc(x0, "x0"))
            for n_, v in (("e", e), ("sa", sa), ("s1m", s1m)):
                put(n_, f32(v, n_))
            if kind == "resblock":
                put("temb_all", f32(temb_all, "temb_all"))
                out["d_temb_all"] = put("d_temb_all", f32(d_temb_all, "d_temb_all"))
                if x1 is not None:
                    x1d = put("x1", nhwc(x1, "x1"))
                    io.c1 = int(x1.shape[1])
            if kind != "input":
                dx0d = put("dx0", nhwc(dx0, "dx0") if dx0 is not None else torch.zeros_like(xd)) if not (kind == "conv" and index == 0) else None
                io.dx0_set = int(dx0 is not None)
                if x1 is not None:
                    dx1d = put("dx1", nhwc(dx1, "dx1") if dx1 is not None else torch.zeros_like(x1d))
                    io.dx1_set = int(dx1 is not None)
            if kind == "head":
                out["out"] = put("out_nchw", torch.empty(B, int(m.out_ch), H, W, device=dev))
                out["loss"] = put("loss", torch.zeros(1, device=dev))
            else:
                names = self.stage_names("conv" if kind == "input" else kind)
                name = names[0 if kind == "input" else index]
                cout = self.layout[name + (".conv2.weight" if kind == "resblock" else ".proj_out.weight" if kind == "attn" else ".weight")][1][0]
                sc = (0.5 if ".downsample." in name else 2 if ".upsample." in name else 1) if kind == "conv" else 1
                y = put("y", torch.empty(B, int(H * sc), int(W * sc), cout, dtype=dt, device=dev))
                if dy is not None:
                    dyd = put("dy", nhwc(dy, "dy"))
                    if tuple(dyd.shape) != tuple(y.shape):
                        raise ValueError(f"Trainer.stage: dy has shape {tuple(dyd.shape)} (NHWC), the stage's output {tuple(y.shape)}")
                elif kind != "input":
                    raise ValueError("Trainer.stage: dy is required")
        with torch.cuda.device(dev):
            if kind == "resblock" and (self.dropout > 0.0 or self._dropout_armed):
                _lib.check(L.wdm_trainer_set_dropout(self._t, self.dropout, self.rank_dropout_seed(), self.step + 1))
                self._dropout_armed = self.dropout > 0.0
            n = int(L.wdm_trainer_stage_workspace_bytes(self._t, code, int(index), B, H, W))
            if n == 0:
                raise RuntimeError("wdm_trainer_stage_workspace_bytes failed: " + L.wdm_last_error().decode(errors="replace"))
            ws = torch.empty(n + 256, dtype=torch.uint8, device=dev)
            _lib.check(L.wdm_trainer_stage(self._t, code, int(index), C.byref(io), B, H, W, _lib.ptr(ws), n, _lib.stream_ptr()))
        if kind == "input":
            out["x96"] = back(x96)
        if kind not in ("temb", "head"):
            out["y"] = back(y)
        if kind not in ("temb", "input") and dx0d is not None:
            out["dx0"] = back(dx0d)
        if kind == "resblock" and x1 is not None:
            out["dx1"] = back(dx1d)
        return out

    # ---- dropout ------------------------------------------------------------------------------------------------------
    def _ensure_dropout_seed(self):
        if self.dropout_seed is None:
            self.dropout_seed = int(torch.randint(0, _MASK63, (1,), dtype=torch.int64).item())
        return self.dropout_seed

    def rank_dropout_seed(self):
        """The seed this process draws with: dropout_rank_seed(base seed, rank in the default process group)."""
        import torch.distributed as dist
        self._ensure_dropout_seed()
        rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        return dropout_rank_seed(self.dropout_seed, rank)

    def dropout_blocks(self, R=None):
        """[(block name, layer index, channels, map side)] of the ResnetBlocks in the library's construction order (down, mid, up) for R x R inputs."""
        R = int(R if R is not None else self.config.data.image_size)
        nres = len(self.config.model.ch_mult)
        out = []
        for k, (_, shape) in self.layout.items():
            if k.endswith(".norm2.weight"):
                name = k[:-len(".norm2.weight")]
                level = nres - 1 if name.startswith("mid.") else int(name.split(".")[1])
                out.append((name, len(out), int(shape[0]), R >> level))
        return out

    def dropout_masks(self, B, R=None):
        """{block name: (B, C, H, W) tensor of factors, 0 or 1 / (1 - p)} that the NEXT loss_and_grads call of this process applies behind silu(norm2(.)) of each
        ResnetBlock, from the device function the kernels draw with (wdm_dropout_mask).  Every factor is 1.0 when model.dropout is 0."""
        L, h = _lib.lib(), _lib.handle(self.device.index or 0)
        seed = self.rank_dropout_seed() if self.dropout > 0.0 else 0        # (p = 0: every factor is 1 whatever the seed -- and no seed is drawn for looking)
        out = OrderedDict()
        with torch.cuda.device(self.device):
            for name, layer, ch, side in self.dropout_blocks(R):
                m = torch.empty(int(B), ch, side, side, device=self.device)
                _lib.check(L.wdm_dropout_mask(h, self.dropout, seed, self.step + 1, layer, int(B), side, side, ch, _lib.ptr(m), _lib.stream_ptr()))
                out[name] = m
        return out

    def allreduce_grads(self, group=None):
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            dist.all_reduce(self.grads, op=dist.ReduceOp.SUM, group=group)
            self.grads.div_(dist.get_world_size(group))              # DDP averages

    # ---- gradient all-reduce in buckets that overlap the backward (what DistributedDataParallel does for the reference, ddm_wavelet.py:168) ----------------
    def enable_grad_buckets(self, n: int = 8):
        """The next loss_and_grads calls record an event behind the last launch that writes each of (at most) n buckets of the flat gradient buffer --
        it fills from its end while the backward runs -- so that allreduce_grads_overlapped can start a bucket's all-reduce before the backward is over.
        n = 0 switches it off; n is clamped to the C API's limit of 64 buckets."""
        import ctypes as C
        n = max(0, min(64, int(n)))
        with torch.cuda.device(self.device):
            self._gev = [torch.cuda.Event() for _ in range(int(n))]
            for ev in self._gev:
                ev.record()                                           # torch creates the handle on first use
            arr = (C.c_void_p * max(1, len(self._gev)))(*[C.c_void_p(int(ev.cuda_event)) for ev in self._gev])
            _lib.check(_lib.lib().wdm_trainer_set_grad_events(self._t, arr, len(self._gev)))
            self._comm_stream = torch.cuda.Stream(device=self.device) if self._gev else None

    def grad_buckets(self):
        """[(lo, hi)] in elements of self.grads, in the order the backward completes them (the last step's cut)."""
        import ctypes as C
        n = len(getattr(self, "_gev", []) or [])
        if n == 0:
            return []
        bounds, nb = (C.c_int64 * (n + 1))(), C.c_int()
        _lib.check(_lib.lib().wdm_trainer_grad_buckets(self._t, bounds, n + 1, C.byref(nb)))
        return [(int(bounds[k + 1]), int(bounds[k])) for k in range(nb.value)]

    def allreduce_grads_overlapped(self, group=None):
        """Call right behind loss_and_grads (which only ENQUEUES the step): bucket k's all-reduce waits for its event on a side stream and runs while
        the main stream is still in the backward; the embedding-MLP / temb_proj gradients, final only at the end of the step, follow the whole step.
        Same sums as allreduce_grads (a bucket is a slice of the same buffer)."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1):
            return
        buckets = self.grad_buckets()
        if not buckets:
            return self.allreduce_grads(group)
        main, side = torch.cuda.current_stream(self.device), self._comm_stream
        works = []
        with torch.cuda.stream(side):
            for k, (lo, hi) in enumerate(buckets):
                side.wait_event(self._gev[k])
                works.append(dist.all_reduce(self.grads[lo:hi], op=dist.ReduceOp.SUM, group=group, async_op=True))
            side.wait_stream(main)                                    # the rest is final when the whole step is
            lo_all, hi_all = buckets[-1][0], buckets[0][1]
            if lo_all > 0:
                works.append(dist.all_reduce(self.grads[:lo_all], op=dist.ReduceOp.SUM, group=group, async_op=True))
            if hi_all < self.grads.numel():
                works.append(dist.all_reduce(self.grads[hi_all:], op=dist.ReduceOp.SUM, group=group, async_op=True))
            for w in works:
                w.wait()
        main.wait_stream(side)
        self.grads.div_(dist.get_world_size(group))

    # ---- the guard of the step -------------------------------------------------------------------------
    @property
    def grad_norm(self):
        """Global 2-norm of the last guarded step's gradient (after the all-reduce), a 0-dim device tensor: reading it here causes no wait.  None without a guard."""
        return self._guard.norm if self._guard is not None else None

    @property
    def clip_coef(self):
        """The factor the last guarded step scaled its gradient by: min(1, grad_clip / (norm + 1e-6)), 1 with clipping off.  Device tensor; None without a guard."""
        return self._guard.coef if self._guard is not None else None

    @property
    def skipped_steps(self):
        """How many steps skip_nonfinite has dropped so far (reads the device counter: this one waits)."""
        return self._guard.skipped_steps if self._guard is not None else 0

    def _guarded_optimizer_step(self):
        """optimizer_step behind the guard: the norm of self.grads, then the rule's guarded kernel, which reads the record on the device.  self.step counts calls -- a
        skipped step advances it too (bias corrections, dropout counters, checkpoints and schedules count calls; the device alone knows that the step was dropped).
        SGD: a skipped first step leaves the zero-initialised momentum buffer alone, and the next step's momentum * 0 + g is the buffer it would have created."""
        self._guard.run()
        if self.rule == "adam":         # the unguarded Adam entry takes its hyper-parameters as floats: the same values here
            f32 = lambda v: C.c_float(v).value
            args = (self.step, f32(self.lr), f32(self.betas[0]), f32(self.betas[1]), f32(self.eps), f32(self.weight_decay), f32(self.ema_mu))
        else:
            b1, b2 = {"amsgrad": self.betas, "rmsprop": (0.0, self.alpha), "sgd": (self.momentum, 0.0)}[self.rule]
            step = self.step
            if self.rule == "sgd":
                step = 1 if self._momentum_fresh else max(2, self.step)
                self._momentum_fresh = False
            args = (step, self.lr, b1, b2, self.eps, self.weight_decay, self.ema_mu)
        _lib.check(_lib.lib().wdm_trainer_optim_step_guarded(self._t, *args, self._guard.ptr, _lib.stream_ptr()))

    def optimizer_step(self):
        self.step += 1
        with torch.cuda.device(self.device):
            if self._guard is not None:
                return self._guarded_optimizer_step()
            if self.rule == "adam":
                _lib.check(_lib.lib().wdm_trainer_adam_ema(self._t, self.step, self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay, self.ema_mu,
                                                           _lib.stream_ptr()))
                return
            # the library's first / second decay: Adam's betas, SGD's momentum, RMSProp's alpha (include/wavedm.h)
            b1, b2 = {"amsgrad": self.betas, "rmsprop": (0.0, self.alpha), "sgd": (self.momentum, 0.0)}[self.rule]
            step = self.step
            if self.rule == "sgd":                      # step 1 is the one that creates the buffer, whatever this trainer's count says (torch's SGD keeps none)
                step = 1 if self._momentum_fresh else max(2, self.step)
                self._momentum_fresh = False
            _lib.check(_lib.lib().wdm_trainer_optim_step(self._t, step, self.lr, b1, b2, self.eps, self.weight_decay, self.ema_mu, _lib.stream_ptr()))

    def train_step(self, x0, group=None, generator=None):
        """The body of the reference's loop for one batch of wavelet-domain samples x0 (B,Cin,R,R): noise (model.out_ch channels), antithetic timesteps
        (ddm_wavelet.py:249-256), loss, backward, all-reduce, [the guard, taken behind the all-reduce and its division: every rank reduces the same buffer to the same
        coefficient and the same skip decision, and a NaN on one rank reaches all through the sum -- no collective is added,] optimizer, EMA.  Returns the loss (device tensor)."""
        n = x0.shape[0]
        e = torch.randn((n, int(self.config.model.out_ch)) + tuple(x0.shape[2:]), device=self.device, generator=generator)
        t = torch.randint(low=0, high=self.num_timesteps, size=(n // 2 + 1,), device=self.device, generator=generator)
        t = torch.cat([t, self.num_timesteps - t - 1], dim=0)[:n]
        loss = self.loss_and_grads(x0, t, e)
        if getattr(self, "_gev", None):
            self.allreduce_grads_overlapped(group)
        else:
            self.allreduce_grads(group)
        self.optimizer_step()
        return loss

    # ---- the step fed from images resident in HBM (device_data.py) --------------------------------------------------------------------
    def _ensure_data_seed(self):
        if self.data_seed is None:
            from .device_data import draw_data_seed
            self.data_seed = draw_data_seed()
        return self.data_seed

    def restore_data_seed(self, seed):
        """--resume: the checkpoint's 'data_seed' (None -- a checkpoint without the key -- changes nothing: a seed is drawn when the store is first used)."""
        if seed is not None:
            self.data_seed = int(seed) & _MASK63

    def broadcast_data_seed(self, src=0, group=None):
        """Every rank draws from rank `src`'s seed (the ranks' items differ by their global item numbers, not by their seeds)."""
        import torch.distributed as dist
        self._ensure_data_seed()
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            st = torch.tensor([self.data_seed], device=self.device, dtype=torch.int64)
            dist.broadcast(st, src=src, group=group)
            self.data_seed = int(st.item())
        return self.data_seed

    def store_draw(self, store, group=None, step=None, augment=None):
        """The (img, row, col) triples of the samples optimizer step `step` (default: the next one) takes on this rank: training.batch_size items of
        training.patch_n crops of data.patch_size pixels, a function of (data_seed, step, rank, world) alone (device_data.first_item).  Under data.augment
        (or the keyword, which wins) other than "none": (triples, orientation codes), a function of the mode as well."""
        import torch.distributed as dist
        from .device_data import augment_mode, first_item
        world, rank = (dist.get_world_size(group), dist.get_rank(group)) if (dist.is_available() and dist.is_initialized()) else (1, 0)
        b, patch_n = int(self.config.training.batch_size), int(self.config.training.patch_n)
        g0 = first_item(self.step + 1 if step is None else step, world, rank, b)
        mode = augment_mode(self.config, augment)
        if mode == "none":
            return store.draw(self._ensure_data_seed(), g0, b, patch_n, int(self.config.data.patch_size))
        return store.draw(self._ensure_data_seed(), g0, b, patch_n, int(self.config.data.patch_size), augment=mode)

    def sample_from_store(self, store, group=None, other_bands=None, step=None, augment=None):
        """x0 of the next step, drawn and cut on the device: assemble_training_sample's tensor without a float crop, a second DWT launch or a cat.  With
        model.use_gt_in_train: False the kernel also writes the [0,1] crops and `other_bands(input crops (n,3,p,p)) -> (n,48,p/4,p/4)` supplies the bands from
        other_channels_begin on (DenoisingDiffusion_Wavelet passes its HFRM -> DWT(2x - 1) path).  Under data.augment (or `augment`) every crop takes its drawn
        orientation inside the gather; the HFRM then sees the oriented crops."""
        from .device_data import augment_mode
        m = self.config.model
        if getattr(self.config.data, "global_attn", False):
            raise NotImplementedError("the device-resident data path does not feed the data.global_attn model: it needs `total`, the whole resized image, which the store does not keep")
        if not m.use_other_channels:
            raise NotImplementedError("training with model.use_other_channels: False is not built (DenoisingDiffusion_Wavelet.assemble_training_sample)")
        mode = augment_mode(self.config, augment)
        kw = {}                                                                 # `none`: the calls, kernels and arguments of a run without the key
        if mode == "none":
            triples = self.store_draw(store, group, step, augment=mode)
        else:
            triples, kw["orient"] = self.store_draw(store, group, step, augment=mode)
        p, pc, ob = int(self.config.data.patch_size), int(m.pred_channels), int(m.other_channels_begin)
        if getattr(m, "use_gt_in_train", True) or ob >= 48:
            return store.gather_training_samples(triples, p, pc, ob, **kw)
        if other_bands is None:
            raise ValueError("Trainer.sample_from_store: model.use_gt_in_train: False needs other_bands (the HFRM path of assemble_training_sample)")
        head, crops = store.gather_training_samples(triples, p, pc, 48, want_crops=True, **kw)
        with torch.no_grad():
            other = other_bands(crops[:, :3].contiguous())
        return torch.cat([head, other[:, ob:]], dim=1).contiguous()

    def train_step_from_store(self, store, group=None, generator=None, other_bands=None, augment=None):
        """train_step on samples drawn and cut from a DeviceImageStore: two launches (wdm_data_draw, wdm_train_sample_gather; their *_oriented forms under
        data.augment / `augment`) in front of the unchanged step; noise and timesteps come from torch's device generator exactly as in train_step."""
        return self.train_step(self.sample_from_store(store, group, other_bands, augment=augment), group=group, generator=generator)

    # ---- optimizer state in torch.optim.Adam's state_dict layout (what the reference saves and restores, ddm_wavelet.py:186, :288) ---------
    def param_order(self):
        """Parameter names in the reference's `model.parameters()` order: torch.optim indexes its state by that position."""
        return [k for k, _ in reference_param_order([(k, v[1]) for k, v in self.layout.items()]) if k in self.layout]

    def current_optimizer_spec(self):
        """This trainer's optimizer in optimizer_spec's form (the configured rule with the hyper-parameters in force)."""
        return {"rule": self.rule, "lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay, "alpha": self.alpha,
                "momentum": self.momentum}

    def optimizer_state_dict(self):
        """torch.optim.{Adam, RMSprop, SGD}.state_dict() of the configured optimizer (torch_optimizer_state_dict)."""
        names = self.param_order()
        tensors = {s: [self._view(buf, k).detach().cpu().clone() for k in names] for s, buf in self.opt_state.items()}
        return torch_optimizer_state_dict(self.current_optimizer_spec(), self.step, tensors)

    def load_optimizer_state_dict(self, osd):
        """Accepts the state_dict() of the torch.optim object the configured optimizer is (the reference's checkpoints and this trainer's) and, for Adam, this
        trainer's round-1 flat format.  A checkpoint of another optimizer is a ValueError."""
        if not osd:
            return False
        if "state" in osd and "param_groups" in osd:
            found = _checkpoint_rule(osd)
            if found is not None and found != self.rule:
                raise ValueError(f"the checkpoint holds the state of torch.optim.{_RULE_TITLES[found]}, this trainer is configured for torch.optim.{_RULE_TITLES[self.rule]} "
                                 "(optim.optimizer / optim.amsgrad)")
            names = self.param_order()
            st = osd["state"]
            if len(st) == 0:
                return False
            if len(st) != len(names):
                raise RuntimeError(f"optimizer state holds {len(st)} parameters, the model {len(names)}")
            g = osd["param_groups"][0]
            if self.rule == "rmsprop" and (float(g.get("momentum", 0.0)) != 0.0 or g.get("centered", False)):
                raise NotImplementedError("RMSprop with momentum or centered: the reference's call sets neither (utils/optimize.py:10)")
            if self.rule == "sgd" and (float(g.get("dampening", 0.0)) != 0.0 or g.get("nesterov", False)):
                raise NotImplementedError("SGD with dampening or Nesterov momentum: the reference's call sets neither (utils/optimize.py:12)")
            step = None
            for i, k in enumerate(names):
                e = st[i]
                for s, buf in self.opt_state.items():
                    if tuple(e[s].shape) != self.layout[k][1]:
                        raise RuntimeError(f"optimizer state {i} has shape {tuple(e[s].shape)}, parameter {k} {self.layout[k][1]}")
                    self._view(buf, k).copy_(e[s].to(self.device, torch.float32))
                if "step" in e:
                    step = int(float(e["step"])) if step is None else step
            self.lr, self.weight_decay = float(g["lr"]), float(g["weight_decay"])
            if self.rule in ("adam", "amsgrad"):
                self.eps, self.betas = float(g["eps"]), (float(g["betas"][0]), float(g["betas"][1]))
            elif self.rule == "rmsprop":
                self.eps, self.alpha = float(g["eps"]), float(g["alpha"])
            else:
                self.momentum = float(g["momentum"])
                self._momentum_fresh = False
            if step is not None:
                self.step = step
            return True
        if "exp_avg" in osd and "exp_avg_sq" in osd:                # round-1 format of this repository: the two flat buffers
            if self.rule != "adam":
                raise ValueError(f"the checkpoint holds flat Adam moments, this trainer is configured for torch.optim.{_RULE_TITLES[self.rule]}")
            self.exp_avg.copy_(osd["exp_avg"].to(self.device))
            self.exp_avg_sq.copy_(osd["exp_avg_sq"].to(self.device))
            self.step = int(osd.get("step", self.step))
            return True
        raise RuntimeError("unrecognised optimizer state in the checkpoint")

    def save_checkpoint(self, path, epoch=0):
        """The reference's checkpoint dict (ddm_wavelet.py:282-292): its own `load_ddm_ckpt` (:180-190) reads this file -- it looks up named keys only, so the
        one key added here, 'dropout_seed' (the BASE seed: a resumed run continues with the masks the uninterrupted run would have drawn), does not disturb it."""
        ck = {"epoch": epoch, "step": self.step, "state_dict": {k: v.cpu() for k, v in self.state_dict().items()},
              "optimizer": self.optimizer_state_dict(),
              "ema_helper": {k: v.cpu() for k, v in self.ema_state_dict().items()}, "params": None, "config": None,
              "dropout_seed": self.dropout_seed}                                # (None from a trainer that never used dropout: resumes like a file without the key)
        if self.data_seed is not None:                                          # only a trainer fed from a DeviceImageStore has one: every other checkpoint keeps its keys
            ck["data_seed"] = self.data_seed
        torch.save(ck, path)

    def restore_dropout_seed(self, seed):
        """--resume: take the checkpoint's base seed; a checkpoint without one (the reference's, or an older one of this package) keeps the fresh seed drawn at
        construction, and a run that uses dropout says so once."""
        if seed is not None:
            self.dropout_seed, self._dropout_seed_fresh = int(seed) & _MASK63, False
        elif self.dropout > 0.0 and self._dropout_seed_fresh:
            self._announce_fresh_seed = True                       # said by announce_dropout_seed, once the ranks agree on the seed
            self._dropout_seed_fresh = False

    def announce_dropout_seed(self):
        """Behind broadcast_state: rank 0 says -- once -- that the resumed checkpoint held no seed, with the base seed every rank now uses."""
        import torch.distributed as dist
        if getattr(self, "_announce_fresh_seed", False):
            self._announce_fresh_seed = False
            if not (dist.is_available() and dist.is_initialized()) or dist.get_rank() == 0:
                print(f"wavedm_amd.Trainer: the checkpoint holds no 'dropout_seed'; continuing with a fresh one ({self.dropout_seed})")

    def broadcast_state(self, src=0, group=None):
        """What DistributedDataParallel does at construction (ddm_wavelet.py:168): every rank starts from rank `src`'s parameters (and here
        also its EMA shadow and optimizer state, so that a resumed run is identical on every rank)."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            for buf in (self.params, self.ema, *self.opt_state.values()):
                dist.broadcast(buf, src=src, group=group)
            st = torch.tensor([self.step, -1 if self.dropout_seed is None else self.dropout_seed, int(self._momentum_fresh)], device=self.device, dtype=torch.int64)
            dist.broadcast(st, src=src, group=group)
            self.step = int(st[0].item())
            self._momentum_fresh = bool(st[2].item())
            self.dropout_seed = None if int(st[1].item()) < 0 else int(st[1].item())  # one base seed; each rank draws with dropout_rank_seed(base, its rank)

"""HFRM training in mixed precision (HFRMTrainer(dtype="bf16-mixed"): bf16 activations and GEMMs over fp32 parameters, gradients and Adam
state) on the GPU.  The yardstick of every accuracy bound is another mixed-precision run of the same network on the same GPU -- torch.autocast
bf16 autograd of the oracle, or the bf16 inference HFRM -- measured against the same exact reference (float64 autograd on the CPU, the fp32
inference HFRM, the fp32 trainer): e_hip <= 2 * e_yardstick + 2^-8.  The factor 2 covers rounding points and summation orders, which
legitimately differ between two correct mixed-precision implementations; 2^-8 is bf16's unit roundoff and covers what the yardstick happens
not to round.  Every case prints its figures before it asserts (pytest -s shows them)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, rel_linf
from oracle import wavedm_oracle as O
from wavedm_amd import _lib
from wavedm_amd import procedural as P
from wavedm_amd.arch import HFRM
from wavedm_amd.hfrm_training import HFRM_DEFAULTS, HFRMTrainer, hfrm_lr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U = 2.0 ** -8                                       # bf16 unit roundoff
SMALL = dict(in_channel=3, dim=32, mid_blk_num=1, enc_blk_nums=(1, 1), dec_blk_nums=(1, 1))
ARCHS = {"default": HFRM_DEFAULTS, "small": SMALL}
# (1, 96, 160): 60 rows at the deepest level, no multiple of the 16-row GEMM grid; (3, 48, 80): 45 rows there, an odd count, and three images
# show any bleed of the depthwise halo across image borders
SHAPES = {"1x96x160": (1, 3, 96, 160), "3x48x80": (3, 3, 48, 80)}


def oracle_kw(arch):
    a = ARCHS[arch]
    return dict(enc_blk_nums=tuple(a["enc_blk_nums"]), mid_blk_num=a["mid_blk_num"], dec_blk_nums=tuple(a["dec_blk_nums"]))


@functools.lru_cache(maxsize=None)
def state(arch):
    a = ARCHS[arch]
    return P.procedural_hfrm_state_dict(seed=61, mid_blk_num=a["mid_blk_num"], enc_blk_nums=tuple(a["enc_blk_nums"]), dec_blk_nums=tuple(a["dec_blk_nums"]))


def trainer(arch, dtype, sd=None):
    tr = HFRMTrainer(**ARCHS[arch], dtype=dtype)
    tr.load_state_dict(state(arch) if sd is None else sd, strict=True)
    return tr


@functools.lru_cache(maxsize=None)
def gradient_case(arch, shape_key):
    """x, dy, and per parameter: float64 autograd on the CPU (the reference) and autocast bf16 autograd on the GPU (the yardstick), computed once."""
    shape = SHAPES[shape_key]
    sd = state(arch)
    gen = torch.Generator().manual_seed(5)
    x = torch.rand(shape, generator=gen)
    dy = torch.randn(shape, generator=gen)
    with torch.enable_grad():                   # (other test modules switch autograd off globally)
        sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
        out64 = O.hfrm_forward(sd64, x.double(), **oracle_kw(arch))
        g64 = torch.autograd.grad(out64, list(sd64.values()), grad_outputs=dy.double())
        ps = {k: v.to(DEV).requires_grad_(True) for k, v in sd.items()}
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out_ac = O.hfrm_forward(ps, x.to(DEV), **oracle_kw(arch))
        g_ac = torch.autograd.grad(out_ac, list(ps.values()), grad_outputs=dy.to(DEV).to(out_ac.dtype))
    return x, dy, out64.detach(), [g.detach() for g in g64], [g.detach().double().cpu() for g in g_ac]


def rel_l2(g, ref):
    return float((g.double() - ref).norm() / ref.norm().clamp_min(1e-300))


@pytest.mark.parametrize("shape_key", sorted(SHAPES))
@pytest.mark.parametrize("arch", sorted(ARCHS))
def test_gradients_against_float64_within_twice_autocast(arch, shape_key):
    """Measured on one MI355X (worst tensor by e_hip / (2 e_autocast + 2^-8), and the largest e of each side over all tensors); the full
    table of a run is profiles/hfrm_mixed_parity.md."""
    x, dy, out64, g64, g_ac = gradient_case(arch, shape_key)
    tr = trainer(arch, "bf16-mixed")
    tr.backward_from(x.to(DEV), dy.to(DEV))
    got = tr.grad_dict()
    names = list(state(arch))
    assert list(got) == names and len(names) == len(g64) and (arch != "default" or len(names) == 448)
    rows = []
    for k, ref, ac in zip(names, g64, g_ac):
        assert float(ref.norm()) > 0, k
        e_hip, e_ac = rel_l2(got[k].cpu(), ref), rel_l2(ac, ref)
        rows.append((e_hip / (2 * e_ac + U), k, e_hip, e_ac))
    worst = max(rows)
    print(f"\nPARITY {arch} {shape_key}: tensors {len(rows)}  max e_hip {max(r[2] for r in rows):.3e}  max e_autocast {max(r[3] for r in rows):.3e}  "
          f"worst e_hip / (2 e_autocast + 2^-8) = {worst[0]:.3f} at {worst[1]} (e_hip {worst[2]:.3e}, e_autocast {worst[3]:.3e})  "
          f"max e_hip / e_autocast = {max(r[2] / r[3] for r in rows):.3f}")
    bad = [(k, e_hip, e_ac) for ratio, k, e_hip, e_ac in rows if e_hip > 2 * e_ac + U]
    for k, e_hip, e_ac in bad:
        print(f"PARITY-FAIL {arch} {shape_key} {k}: e_hip {e_hip:.4e} e_autocast {e_ac:.4e} bound {2 * e_ac + U:.4e}")
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("shape", [(2, 3, 64, 96), (1, 3, 96, 160), (3, 3, 48, 80)])
def test_forward_against_bf16_inference(shape):
    sd = state("default")
    x = torch.rand(shape, generator=torch.Generator().manual_seed(9)).to(DEV)
    gt = torch.rand(shape, generator=torch.Generator().manual_seed(10)).to(DEV)
    _, out = trainer("default", "bf16-mixed").loss_and_grads(x, gt, return_output=True)
    outs = {}
    for dtype in ("f32", "bf16"):
        m = HFRM(**HFRM_DEFAULTS, dtype=dtype)
        m.load_state_dict(sd, strict=True)
        with torch.no_grad():
            outs[dtype] = m.to(DEV)(x).float().cpu()
    e_tr, e_inf = rel_linf(out.cpu(), outs["f32"]), rel_linf(outs["bf16"], outs["f32"])
    print(f"\nFORWARD {shape}: rel_linf trainer {e_tr:.3e}  inference bf16 {e_inf:.3e}")
    assert e_tr <= 2 * e_inf + U, (e_tr, e_inf)


def test_reference_init_gradients_are_exact_zeros_inside_blocks():
    """weights_init_normal: every block is the identity and beta = gamma = 0, so inside the blocks only beta / gamma get a gradient; the zeros
    are exact in bf16 too (0 * finite = 0, and no rounding makes a zero non-zero)."""
    gen = torch.Generator().manual_seed(21)
    x = torch.rand(2, 3, 64, 96, generator=gen).to(DEV)
    gt = torch.rand(2, 3, 64, 96, generator=gen).to(DEV)
    tr = HFRMTrainer(**HFRM_DEFAULTS, dtype="bf16-mixed")
    tr.init_reference(3)
    loss = float(tr.loss_and_grads(x, gt))
    assert np.isfinite(loss) and loss > 0
    grads = tr.grad_dict()
    for n, v in grads.items():
        if n.startswith(("encoders.", "decoders.", "mid_blks.")) and not n.endswith((".beta", ".gamma")):
            assert int(torch.count_nonzero(v)) == 0, n
    assert all(float(grads[n].abs().max()) > 0 for n in grads if n.endswith((".beta", ".gamma")))
    assert all(float(grads[n].abs().max()) > 0 for n in ("conv_in.weight", "conv_in.bias", "conv_out.weight", "conv_out.bias"))


def test_step_is_deterministic_and_modes_do_not_leak():
    gen = torch.Generator().manual_seed(13)
    x = torch.rand(2, 3, 64, 96, generator=gen).to(DEV)
    gt = torch.rand(2, 3, 64, 96, generator=gen).to(DEV)
    tr = trainer("default", "f32")
    assert tr.precision == "f32"
    l32 = tr.loss_and_grads(x, gt).clone()
    g32 = tr.grads.clone()
    tr.set_precision("bf16-mixed")
    assert tr.precision == "bf16-mixed"
    l1 = tr.loss_and_grads(x, gt).clone()
    g1 = tr.grads.clone()
    l2 = tr.loss_and_grads(x, gt).clone()
    assert torch.equal(l1, l2) and torch.equal(g1, tr.grads)
    assert not torch.equal(g1, g32)                       # (the mode did switch)
    tr.set_precision("f32")
    l3 = tr.loss_and_grads(x, gt).clone()
    assert torch.equal(l3, l32) and torch.equal(tr.grads, g32)
    fresh = trainer("default", "bf16-mixed")              # a trainer created in the mode computes what the switched one did
    assert torch.equal(fresh.loss_and_grads(x, gt), l1) and torch.equal(fresh.grads, g1)


def test_five_train_steps_follow_the_fp32_trainer():
    sd = state("default")
    gen = torch.Generator().manual_seed(12)
    x = torch.rand(2, 3, 64, 96, generator=gen).to(DEV)
    gt = (x * 0.8 + 0.1 * torch.rand(2, 3, 64, 96, generator=gen).to(DEV)).contiguous()
    losses = {}
    for dtype in ("f32", "bf16-mixed"):
        tr = trainer("default", dtype)
        losses[dtype] = [float(tr.train_step(x, gt)[0]) for _ in range(5)]
        assert tr.step == 5

    def eager(autocast):
        ps = {k: v.clone().to(DEV).requires_grad_(True) for k, v in sd.items()}
        opt = torch.optim.Adam(list(ps.values()), lr=2e-4, betas=(0.5, 0.999))
        out = []
        for step in range(1, 6):
            for grp in opt.param_groups:
                grp["lr"] = hfrm_lr(step)
            opt.zero_grad()
            with torch.enable_grad():
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                    y = O.hfrm_forward(ps, x)
                loss = torch.mean(torch.abs(y.float() * 255 - gt * 255)) * 2
                loss.backward()
            opt.step()
            out.append(float(loss.detach()))
        return out
    e32, eac = eager(False), eager(True)
    ours, base = losses["bf16-mixed"], losses["f32"]
    print(f"\nSTEPS mixed {ours}\nSTEPS f32 trainer {base}\nSTEPS eager f32 {e32}\nSTEPS eager autocast {eac}")
    assert ours[-1] < ours[0], ours
    for i in range(5):
        dev, allowed = abs(ours[i] - base[i]), 2 * abs(eac[i] - e32[i]) + U * abs(base[i])
        print(f"STEPS step {i + 1}: |mixed - f32| = {dev:.4e}   2 |autocast - eager| + 2^-8 |f32| = {allowed:.4e}")
    for i in range(5):
        assert abs(ours[i] - base[i]) <= 2 * abs(eac[i] - e32[i]) + U * abs(base[i]), (i, ours, base, eac, e32)


def test_workspace_is_exact_and_checked_before_the_first_launch():
    L = _lib.lib()
    B, H, W = 2, 64, 96
    gen = torch.Generator().manual_seed(14)
    x = torch.rand(B, 3, H, W, generator=gen).to(DEV)
    gt = torch.rand(B, 3, H, W, generator=gen).to(DEV)
    tr32, tr = trainer("default", "f32"), trainer("default", "bf16-mixed")
    n32, n = int(L.wdm_hfrm_trainer_workspace_bytes(tr32._t, B, H, W)), int(L.wdm_hfrm_trainer_workspace_bytes(tr._t, B, H, W))
    print(f"\nWORKSPACE 2x64x96: f32 {n32} bytes, bf16-mixed {n} bytes")
    assert 0 < n < n32
    tr.grads.fill_(7.0)                                   # (the padding between tensors is never written: the same value there on both sides)
    want_loss = tr.loss_and_grads(x, gt).clone()
    want_grads = tr.grads.clone()
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    loss, out = torch.zeros(1, device=DEV), torch.empty_like(gt)

    def step(nbytes):
        return L.wdm_hfrm_trainer_step(tr._t, _lib.ptr(x), _lib.ptr(gt), None, B, H, W, _lib.ptr(loss), _lib.ptr(out), _lib.ptr(ws), nbytes, _lib.stream_ptr())
    tr.grads.fill_(7.0)
    assert step(ws.numel()) == _lib.WDM_OK                 # exactly the queried size
    torch.cuda.synchronize()
    assert torch.equal(loss[0], want_loss) and torch.equal(tr.grads, want_grads)
    tr.grads.fill_(7.0)
    out.fill_(-3.0)
    assert step(ws.numel() - 4096) == _lib.WDM_ENOMEM
    assert b"workspace too small" in L.wdm_last_error()
    torch.cuda.synchronize()
    assert bool((tr.grads == 7.0).all()) and bool((out == -3.0).all())      # refused before anything was launched


def test_checkpoint_moves_between_modes(tmp_path):
    gen = torch.Generator().manual_seed(15)
    x = torch.rand(1, 3, 32, 48, generator=gen).to(DEV)
    gt = torch.rand(1, 3, 32, 48, generator=gen).to(DEV)
    tr = trainer("default", "bf16-mixed")
    tr.train_step(x, gt)
    path = str(tmp_path / "lastest.pth")
    tr.save(path)
    sd = torch.load(path, map_location="cpu")
    assert list(sd) == list(P.hfrm_param_shapes())
    assert all(v.dtype == torch.float32 and tuple(v.shape) == P.hfrm_param_shapes()[k] for k, v in sd.items())
    assert all(torch.equal(sd[k], v.cpu()) for k, v in tr.state_dict().items())
    assert any(not torch.equal(sd[k], state("default")[k]) for k in sd)                 # (the step did move the weights)
    for dtype in ("f32", "bf16"):
        m = HFRM(**HFRM_DEFAULTS, dtype=dtype)
        m.load_state_dict(sd, strict=True)
        got = m.state_dict()
        assert all(torch.equal(got[k].cpu(), sd[k]) for k in sd), dtype
    tr32 = HFRMTrainer(**HFRM_DEFAULTS)
    tr32.load_state_dict(sd, strict=True)
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in tr32.state_dict().items())


def test_train_hfrm_script_mixed_with_sample_sheets(tmp_path):
    from PIL import Image
    root = tmp_path / "data" / "raindrop" / "train"
    (root / "input").mkdir(parents=True)
    (root / "gt").mkdir(parents=True)
    rng = np.random.default_rng(0)
    for k, (w, h) in enumerate([(720, 480), (720, 480), (640, 400)]):
        a = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        b = np.clip(a.astype(np.int16) + rng.integers(-8, 9, size=a.shape), 0, 255).astype(np.uint8)
        Image.fromarray(a).save(root / "input" / f"{k}_rain.png")
        Image.fromarray(b).save(root / "gt" / f"{k}_clean.png")
    save, sheets = tmp_path / "saved", tmp_path / "sheets"
    cmd = [sys.executable, os.path.join(REPO, "scripts", "train_hfrm.py"), "--data_dir", str(tmp_path / "data"), "--save_dir", str(save),
           "--batch_size", "2", "--n_cpu", "0", "--n_epochs", "5", "--max_steps", "3", "--best_psnr", "-1000",
           "--dtype", "bf16-mixed", "--sample_interval", "1", "--sample_dir", str(sheets)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "dtype='bf16-mixed'" in r.stdout and "epoch PSNR" in r.stdout
    for f in ("lastest.pth", "best.pth"):
        sd = torch.load(str(save / "raindrop" / f), map_location="cpu")
        assert list(sd) == list(P.hfrm_param_shapes())
    pngs = sorted(os.listdir(sheets))
    assert len(pngs) == 3 and pngs[0] == "000_000000.png", pngs
    for f in pngs:
        a = np.asarray(Image.open(sheets / f))
        assert a.shape == (480, 3 * 720, 3) and a.dtype == np.uint8
        assert a[:, :720].std() > 10 and a[:, 1440:].std() > 10

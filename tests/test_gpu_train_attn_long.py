"""GPU: the training step of a UNet whose AttnBlocks sit on maps beyond 512 tokens (attn_resolutions [32, 16] on 32 x 32 patches: 1 024-token softmax rows, forward and
backward) -- loss and every gradient against torch autograd over the oracle, bf16 against f32, two steps bit for bit.  `attn: ... tokens unsupported` before."""
import pytest
import torch

from gpu_util import dev, seeded
from oracle import wavedm_oracle as O
from wavedm_amd import _lib
from wavedm_amd import procedural as P
from wavedm_amd.training import Trainer, attn_long_workspace_bytes

pytestmark = pytest.mark.gpu
B = 2


def long_config():
    cfg = P.raindrop_wavelet_config(image_size=32, ch=32, ch_mult=(1, 2), attn_resolutions=(32, 16))
    cfg.device = dev()
    return cfg


@pytest.fixture(scope="module")
def ref():
    """Inputs and torch autograd over the oracle on the host: computed once, never changed."""
    cfg = long_config()
    sd = P.procedural_state_dict(cfg, seed=61)
    x0, e, t = seeded((B, 96, 32, 32), 421), seeded((B, 3, 32, 32), 422), torch.tensor([700, 120])
    ol, _, og = O.train_grads(sd, cfg, x0, t, e, O.beta_schedule(cfg))
    return cfg, sd, x0, e, t, float(ol), og


def _trainer(cfg, sd, dtype):
    tr = Trainer(cfg, dtype=dtype)
    tr.load_state_dict(sd)
    return tr


def test_training_step_f32_matches_the_oracle(ref):
    cfg, sd, x0, e, t, ol, og = ref
    tr = _trainer(cfg, sd, "f32")
    loss = float(tr.loss_and_grads(x0.to(dev()), t, e.to(dev())))
    print(f"attn_resolutions [32, 16] training step f32: loss rel {abs(loss - ol) / abs(ol):.3e}")
    assert abs(loss - ol) <= 1e-4 * abs(ol)
    g = tr.grad_dict()
    assert set(g) == set(og)
    # the floor rule of test_training_step_full_width_f32: gradients that are zero in exact arithmetic (every AttnBlock k.bias) hold rounding noise on both sides
    floor = 1e-4 * max(float(v.abs().max()) for v in og.values())
    worst = ("", 0.0)
    for k in og:
        err = float((g[k].cpu() - og[k]).abs().max()) / max(float(og[k].abs().max()), floor)
        worst = max(worst, (k, err), key=lambda kv: kv[1])
        assert err <= 2e-3, (k, err)
    print(f"attn_resolutions [32, 16] training step f32: worst gradient {worst[0]} {worst[1]:.3e} of {len(og)} tensors")
    assert any(".attn." in k and k.startswith(("down.0.", "up.0.")) for k in og)          # the 1 024-token blocks are among them


def test_training_step_bf16_tracks_f32(ref):
    cfg, sd, x0, e, t, _, _ = ref
    trf, trb = _trainer(cfg, sd, "f32"), _trainer(cfg, sd, "bf16")
    lf, lb = float(trf.loss_and_grads(x0.to(dev()), t, e.to(dev()))), float(trb.loss_and_grads(x0.to(dev()), t, e.to(dev())))
    gf, gb = trf.grads, trb.grads
    cos = float((gf * gb).sum() / (gf.norm() * gb.norm()))
    print(f"attn_resolutions [32, 16] training step bf16 vs f32: loss rel {abs(lf - lb) / abs(lf):.3e}, gradient cosine {cos:.5f}")
    assert abs(lf - lb) <= 2e-2 * abs(lf)
    assert cos >= 0.98, cos


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_two_steps_are_deterministic(ref, dtype):
    cfg, sd, x0, e, t, _, _ = ref
    out = []
    for _ in range(2):
        tr = _trainer(cfg, sd, dtype)
        losses = []
        for step in range(2):
            losses.append(float(tr.loss_and_grads(x0.to(dev()), t, e.to(dev()))))
            tr.optimizer_step()
        out.append((losses, tr.grads.clone(), tr.params.clone()))
    assert out[0][0] == out[1][0] and torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2], out[1][2])
    assert bool(torch.isfinite(out[0][1]).all()) and out[0][0][0] != out[0][0][1]


def test_workspace_too_small_for_the_attention_fails_before_any_launch(ref):
    """wdm_trainer_step counts the AttnBlocks' kept softmax matrices and backward transients first: a workspace that cannot hold them is refused with WDM_ENOMEM
    while the loss and the gradient buffer are still untouched; Trainer sizes its workspace with the same term."""
    cfg, sd, x0, e, t, _, _ = ref
    tr = _trainer(cfg, sd, "f32")
    need = attn_long_workspace_bytes(cfg.model, B, 32, 4)
    # 5 blocks of 1 024 tokens (2 down, 3 up; the mid block has 256): kept P + fp32 dP, dS and two transposed operands of one
    assert need == 5 * B * 1024 * 1024 * 4 + B * 1024 * 1024 * 16
    tr.grads.fill_(3.0)
    tr._loss.fill_(-1.0)
    ws = torch.empty(need // 2, dtype=torch.uint8, device=dev())
    a = (1 - tr.betas_t).cumprod(dim=0).index_select(0, t.to(dev()).long())
    sa, s1m, tf = a.sqrt().contiguous(), (1.0 - a).sqrt().contiguous(), t.to(dev()).float().contiguous()
    xd, ed = x0.to(dev()), e.to(dev())
    rc = _lib.lib().wdm_trainer_step(tr._t, _lib.ptr(xd), _lib.ptr(tf), _lib.ptr(sa), _lib.ptr(s1m), _lib.ptr(ed), B, tr._c_t0, _lib.ptr(tr._loss), None, _lib.ptr(ws),
                                     ws.numel(), _lib.stream_ptr())
    msg = _lib.lib().wdm_last_error().decode(errors="replace")
    torch.cuda.synchronize()
    assert rc == _lib.WDM_ENOMEM and "attention" in msg, (rc, msg)
    assert float(tr._loss[0]) == -1.0 and bool((tr.grads == 3.0).all())

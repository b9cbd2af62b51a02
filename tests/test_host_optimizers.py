"""optim.optimizer / optim.amsgrad without a GPU: `optimizer_spec` against the call utils/optimize.py:5-14 makes for each of the four settings, and the
optimizer state dicts the trainer writes (built from zeros through the trainer's own helper) against torch.optim's load_state_dict."""
from types import SimpleNamespace

import pytest
import torch

from wavedm_amd import procedural as P
from wavedm_amd.training import STATE_NAMES, optimizer_spec, torch_optimizer, torch_optimizer_state_dict


def _config(**optim):
    cfg = P.reduced_config()
    cfg.optim = SimpleNamespace(**dict(dict(optimizer="Adam", amsgrad=False, lr=2e-4, eps=1e-3, weight_decay=0.01), **optim))
    return cfg


def test_spec_adam_takes_every_key_of_the_config():
    # optim.Adam(parameters, lr=lr, weight_decay=weight_decay, betas=(0.9, 0.999), amsgrad=amsgrad, eps=eps)
    s = optimizer_spec(_config())
    assert s["rule"] == "adam" and s["lr"] == 2e-4 and s["eps"] == 1e-3 and s["weight_decay"] == 0.01 and tuple(s["betas"]) == (0.9, 0.999)
    s = optimizer_spec(_config(amsgrad=True))
    assert s["rule"] == "amsgrad" and s["lr"] == 2e-4 and s["eps"] == 1e-3 and s["weight_decay"] == 0.01 and tuple(s["betas"]) == (0.9, 0.999)


def test_spec_rmsprop_keeps_torchs_eps():
    # optim.RMSprop(parameters, lr=lr, weight_decay=weight_decay): optim.eps is not passed
    s = optimizer_spec(_config(optimizer="RMSProp"))
    assert s["rule"] == "rmsprop" and s["lr"] == 2e-4 and s["weight_decay"] == 0.01
    assert s["eps"] == 1e-8 and s["alpha"] == 0.99 and s["momentum"] == 0.0
    ref = torch.optim.RMSprop([torch.nn.Parameter(torch.zeros(1))], lr=2e-4, weight_decay=0.01).defaults
    assert (s["eps"], s["alpha"], s["momentum"]) == (ref["eps"], ref["alpha"], ref["momentum"]) and not ref["centered"]


def test_spec_sgd_drops_the_weight_decay():
    # optim.SGD(parameters, lr=lr, momentum=0.9): optim.weight_decay is not passed
    s = optimizer_spec(_config(optimizer="SGD"))
    assert s["rule"] == "sgd" and s["lr"] == 2e-4 and s["momentum"] == 0.9 and s["weight_decay"] == 0.0
    ref = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=2e-4, momentum=0.9).defaults
    assert ref["weight_decay"] == 0.0 and ref["dampening"] == 0.0 and not ref["nesterov"]


@pytest.mark.parametrize("name", ["rmsprop", "AdamW"])
def test_spec_refuses_other_names_with_the_references_message(name):
    with pytest.raises(NotImplementedError) as e:
        optimizer_spec(_config(optimizer=name))
    assert str(e.value) == "Optimizer {} not understood.".format(name)


def test_spec_of_a_config_without_the_keys_is_the_shipped_adam():
    cfg = P.reduced_config()
    cfg.optim = SimpleNamespace(lr=1e-3, eps=1e-8, weight_decay=0.0)           # (how the training tests write it)
    assert optimizer_spec(cfg)["rule"] == "adam" and optimizer_spec(cfg)["lr"] == 1e-3


@pytest.mark.parametrize("optim", [dict(optimizer="Adam", amsgrad=True), dict(optimizer="RMSProp"), dict(optimizer="SGD")], ids=["amsgrad", "rmsprop", "sgd"])
def test_torch_accepts_the_state_dict_the_trainer_writes(optim):
    spec = optimizer_spec(_config(**optim))
    shapes = list(P.unet_param_shapes(P.reduced_config()).values())
    sd = torch_optimizer_state_dict(spec, 0, {k: [torch.zeros(s) for s in shapes] for k in STATE_NAMES[spec["rule"]]})
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    opt = torch_optimizer(spec, params)
    fresh = opt.state_dict()["param_groups"][0]
    assert set(sd["param_groups"][0]) == set(fresh)                            # the keys torch writes for this optimizer, no more, no fewer
    assert all(sd["param_groups"][0][k] == fresh[k] for k in fresh)
    opt.load_state_dict(sd)
    for k in STATE_NAMES[spec["rule"]]:
        assert tuple(opt.state[params[3]][k].shape) == tuple(shapes[3])
    assert ("step" in opt.state[params[0]]) == (spec["rule"] != "sgd")
    for p in params[:4]:                                                         # and torch steps from it
        p.grad = torch.ones_like(p)
    for p in params[4:]:
        p.grad = torch.zeros_like(p)
    opt.step()
    assert float(params[0].detach().abs().max()) > 0

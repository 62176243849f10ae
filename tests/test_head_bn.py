"""--head mlp_bn without a GPU: the flags, the module tree and its state-dict keys, the refusals,
and that runs without the flag keep the options and keys they had."""
import pytest
import torch

from simclr_pytorch_distributed_amd.config import parse_linear, parse_pretrain
from simclr_pytorch_distributed_amd.models.executor import ModelRunner, head_forward
from simclr_pytorch_distributed_amd.models.resnet import SupConResNet, bn_projector, is_bn_projector

BN_KEYS = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


def head_keys(model):
    return sorted(k for k in model.state_dict() if k.startswith("head."))


@pytest.mark.parametrize("L", [2, 3])
def test_state_dict_keys(L):
    m = SupConResNet("resnet18", head="mlp_bn", feat_dim=64, head_hidden=96, head_layers=L)
    want = [f"head.{3 * i}.weight" for i in range(L)] + [f"head.{3 * i + 1}.{k}" for i in range(L - 1) for k in BN_KEYS]
    assert head_keys(m) == sorted(want)
    assert is_bn_projector(m.head) and m.head[0].weight.shape == (96, 512) and m.head[-1].weight.shape == (64, 96)
    assert SupConResNet("resnet18", head="mlp_bn", feat_dim=64).head[0].out_features == 512   # H defaults to dim_in


def test_flags():
    opt = parse_pretrain(["--head", "mlp_bn", "--head_hidden", "256", "--head_layers", "2", "--feat_dim", "256"],
                         make_dirs=False)
    assert (opt.head, opt.head_hidden, opt.head_layers) == ("mlp_bn", 256, 2)
    assert "head_hidden" not in vars(parse_pretrain(["--head", "mlp_bn", "--feat_dim", "128"], make_dirs=False))
    for bad in (["--head", "mlp_bn", "--micro_batch", "64"], ["--head", "mlp_bn", "--head_hidden", "100"],
                ["--head", "mlp_bn", "--feat_dim", "48"], ["--head_hidden", "256"], ["--head_layers", "2"]):
        with pytest.raises(ValueError):
            parse_pretrain(bad, make_dirs=False)
    with pytest.raises(SystemExit):      # main_supcon.py only
        parse_linear(["--head", "mlp_bn"], make_dirs=False)


def test_default_run_unchanged():
    a, b = vars(parse_pretrain([], make_dirs=False)), vars(parse_pretrain(["--head", "mlp"], make_dirs=False))
    drop = lambda d: {k: v for k, v in d.items() if not k.startswith(("conf_work", "tb_folder", "save_folder"))}  # noqa: E731
    assert drop(a) == drop(b) and not any(k.startswith("head_") for k in a)
    assert head_keys(SupConResNet("resnet18")) == ["head.0.bias", "head.0.weight", "head.2.bias", "head.2.weight"]


def test_torch_path_is_the_sequential():
    torch.manual_seed(0)
    model = SupConResNet("resnet18", head="mlp_bn", feat_dim=32, head_hidden=64)
    feat = torch.randn(12, 512)
    ref = bn_projector(512, 64, 32)
    ref.load_state_dict(model.head.state_dict())
    want = ref(feat)
    got = head_forward(model.head, feat)
    assert torch.equal(got, want) and torch.equal(model.head[1].running_mean, ref[1].running_mean)
    x = torch.randn(4, 3, 32, 32)
    twin = SupConResNet("resnet18", head="mlp_bn", feat_dim=32, head_hidden=64)
    twin.load_state_dict(model.state_dict())
    assert torch.equal(ModelRunner(model, backend="torch", precision="fp32").forward(x), twin(x))

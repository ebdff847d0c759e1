"""The BottleBlock converter (converter_layer != 1) through the Python surface on the GPU: the personalised head against the values
captured from the reference (tests/golden/bce_bottle.npz, client_public_bce_bottle.npz), the eval path, and the callers that take the
head's parameters as a list (FusedHeadTrainer through Client.train_with_public_data, ShardedHeadTrainer)."""
import numpy as np
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

from conftest import load_golden  # noqa: E402
from oracle import ref_cpu as R  # noqa: E402

import bottle_cases as bc  # noqa: E402

from fedfr_amd import backbones, losses, client  # noqa: E402
from fedfr_amd.comm import SingleComm  # noqa: E402
from fedfr_amd.partial_fc import PartialFC  # noqa: E402

DEV = torch.device("cuda:0")


def T(a):
    return torch.from_numpy(np.asarray(a))


def rel(a, b):
    a, b = a.detach().double().cpu(), T(b).double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def maxrel(a, b):
    a, b = a.detach().double().cpu(), T(b).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def load_bottle(converter):
    converter.load_state_dict(dict(zip(bc.PARAM_KEYS, bc.golden_params(512))))


def test_bce_head_with_bottleblock_vs_reference():
    g = load_golden("bce_bottle")
    B, C = int(g["B"]), int(g["C"])
    x = R.closed_form((B, 512), 0.113, 0.2, 1.0).to(DEV).requires_grad_(True)
    mod = client.BCE_module(512, C, 2)
    mod.weight.data = R.closed_form((C, 512), 0.071, 1.1, 0.05)
    mod.bias.data = R.closed_form((C,), 0.5, 0.1, 0.1)
    load_bottle(mod.converter)
    mod.to(DEV)
    assert list(mod.state_dict().keys()) == [str(k) for k in g["keys"]]
    with torch.no_grad():
        assert maxrel(mod.converter(x), g["conv_out"]) < 1e-3
    z, gt = mod(x, T(g["labels"]).to(DEV))
    loss = losses.BCE_loss()(z, gt)
    loss.backward()
    assert maxrel(z, g["z"]) < 1e-3
    assert bool((gt.cpu() == T(g["gt"])).all())
    assert abs(float(loss) - float(g["loss"])) < 1e-3 * abs(float(g["loss"]))
    assert maxrel(x.grad, g["dx"]) < 1e-3
    assert maxrel(mod.weight.grad, g["d_weight"]) < 1e-3
    assert maxrel(mod.bias.grad, g["d_bias"]) < 1e-3
    conv = dict(mod.converter.named_parameters())
    for k in ("br1.0.weight", "br3.2.weight", "concat_fc.weight"):
        assert maxrel(conv[k].grad[:8, :64], g["d_" + k + "_slice"]) < 1e-3, k
    for k, p in conv.items():
        assert abs(float(p.grad.norm()) - float(g["norm_d_" + k])) < 1e-3 * float(g["norm_d_" + k]), k
        if k.endswith("bias"):
            assert maxrel(p.grad, g["d_" + k]) < 1e-3, k


def test_train_with_public_data_bottleblock_vs_reference():
    """tests/test_e2e_gpu.py::test_train_with_public_data_vs_reference[full] with cfg.converter_layer = 2: iresnet18, 6 local + 14 public
    classes, 3 SGD steps of Branch_model + 10 * BCE + mu * contrastive, the converter a BottleBlock with closed-form parameters."""
    g = load_golden("client_public_bce_bottle")
    nl, npub, B, steps = int(g["n_local"]), int(g["n_public"]), int(g["B"]), int(g["steps"])
    layers = R.IRESNET_LAYERS["iresnet18"]

    class Args:
        network, loss, local_epoch, output_dir, aggr_alg, num_client = "iresnet18", "CosFace", 1, "/tmp", "FedAvg", 4
        BCE_local, contrastive_bb, reweight_cosface = True, True, False
        BCE_detach, combine_dataset = False, True

    class DS:
        ID_base, num_classes = 0, nl

    class Loader(list):
        dataset = DS()

    class Data:
        train_class_sizes, train_dataset_sizes, train_loaders = [nl], [B * steps], [Loader()]

    from fedfr_amd.config import config as cfg
    saved = (cfg.lr, cfg.mu, cfg.converter_layer)
    cfg.lr, cfg.mu, cfg.converter_layer = float(g["lr"]), float(g["mu"]), 2
    try:
        cl = client.Client(0, Args, Data, device=DEV)
        assert isinstance(cl.bce_module.converter, backbones.BottleBlock)
        cl.backbone_state_dict = R.closed_form_state_dict(layers, tag=float(g["tag"]))
        cl.fc_module.fc.data = R.head_fc(nl, seed=11)
        cl.bce_module.weight.data = R.head_fc(nl, seed=13)
        load_bottle(cl.bce_module.converter)
        cl.last_model.load_state_dict(R.closed_form_state_dict(layers, tag=float(g["last_tag"])))
        batches = [(R.closed_form_images(B, tag=float(st)), R.closed_form_labels(B, nl + npub, tag=st)) for st in range(steps)]
        cl.train_with_public_data(pretrained_fc=R.head_fc(npub, seed=12), combine_loader=batches)
    finally:
        cfg.lr, cfg.mu, cfg.converter_layer = saved
    rows = g["rows"]
    assert abs(cl.get_train_loss() - rows[:, 0].mean()) < 1e-2 * abs(rows[:, 0].mean()), (cl.get_train_loss(), rows[:, 0].mean())
    assert abs(cl.cos_meter.avg - rows[:, 1].mean()) < 1e-2 * abs(rows[:, 1].mean())
    assert abs(cl.con_meter.avg - rows[:, 2].mean()) < 2e-2 * abs(rows[:, 2].mean()), (cl.con_meter.avg, rows[:, 2].mean())
    assert abs(cl.bce_meter.avg - rows[:, 3].mean()) < 1e-2 * abs(rows[:, 3].mean())
    out = cl.get_model()
    assert int(out["bn1.num_batches_tracked"]) == int(g["sd_bn1.num_batches_tracked"])
    for k in ("bn1.running_mean", "layer4.1.bn3.running_var", "features.running_mean"):
        assert rel(out[k], g["sd_" + k]) < 3e-2, (k, rel(out[k], g["sd_" + k]))
    for k in ("conv1.weight", "layer2.0.downsample.0.weight", "bn1.weight", "prelu.weight", "fc.bias"):
        assert rel(out[k], g["sd_" + k]) < 1e-2, (k, rel(out[k], g["sd_" + k]))
    assert rel(cl.fc_module.fc.data, g["head_fc"]) < 5e-2
    assert rel(cl.bce_module.weight.data, g["bce_weight"]) < 5e-2
    conv = cl.bce_module.converter.state_dict()
    initial = dict(zip(bc.PARAM_KEYS, bc.golden_params(512)))
    for k in ("br1.0.weight", "br3.2.weight", "concat_fc.weight"):
        assert rel(conv[k][:8, :64], g["bce_conv_" + k + "_slice"]) < 1e-2, (k, rel(conv[k][:8, :64], g["bce_conv_" + k + "_slice"]))
        assert not torch.equal(conv[k].cpu(), initial[k]), k                      # the converter was trained
    assert torch.equal(cl.last_model.state_dict()["conv1.weight"].cpu(), out["conv1.weight"].cpu())


def test_eval_path_equals_the_training_forward_and_keeps_no_gradient_state():
    """nn.Sequential(backbone, converter) under no_grad (Client._local_verification, eval_local): the same bits as the autograd-tracked
    forward, no graph and no gradients"""
    bb = backbones.iresnet18(False, dropout=0, fp16=True)
    bb.load_state_dict(R.closed_form_state_dict(R.IRESNET_LAYERS["iresnet18"], tag=2.0))
    conv = backbones.BottleBlock(512, 4)
    load_bottle(conv)
    model = nn.Sequential(bb, conv).to(DEV).eval()
    imgs = R.closed_form_images(8).to(DEV)
    with torch.no_grad():
        feats = bb(imgs)
        emb = model(imgs)
    assert emb.shape == (8, 512) and emb.grad_fn is None and not emb.requires_grad
    assert all(p.grad is None for p in conv.parameters())
    tracked = conv(feats.clone().requires_grad_(True))
    assert tracked.grad_fn is not None
    assert torch.equal(emb, tracked.detach())
    assert bool(torch.isfinite(emb).all()) and not torch.equal(emb, feats)


def test_sharded_head_trainer_step_updates_all_bottleblock_tensors():
    B, C = 8, 64
    bb = backbones.iresnet18(False, dropout=0, fp16=True)
    bb.load_state_dict(R.closed_form_state_dict(R.IRESNET_LAYERS["iresnet18"], tag=1.0))
    bb = bb.to(DEV)
    pfc = PartialFC(rank=0, local_rank=0, world_size=1, batch_size=B, resume=False, margin_softmax=losses.CosFace(s=30, m=0.4),
                    num_classes=C, sample_rate=1.0, embedding_size=512, prefix="/tmp", comm=SingleComm())
    bm = client.BCE_module(512, C, 2)
    load_bottle(bm.converter)
    bm = bm.to(DEV)
    before = [p.detach().clone() for p in bm.converter.parameters()]
    tr = client.ShardedHeadTrainer(bb, pfc, bm, id_base=0, lr=0.01)
    loss, cos_loss, bce = tr.step(R.closed_form_images(B).to(DEV), R.closed_form_labels(B, C).to(DEV))
    tr.finish()
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and np.isfinite(float(bce)) and float(bce) > 0
    for k, p0, p in zip(bc.PARAM_KEYS, before, bm.converter.parameters()):
        assert bool(torch.isfinite(p).all()) and not torch.equal(p0, p.detach()), k

"""Launch pin of the encoder TRAINING path (neural_astar/encoder_train.py): which ``nastar_*`` entry points of the C ABI one
``encode(...)`` + ``backward()`` calls, and how often, in every mode the host code distinguishes -- streamed or padded closing convolution,
with or without the fused activation, split or plain fp16 operands, pooling, the U-Net plan, eval-mode BatchNorm under autograd and the
data-parallel (sync) BatchNorm.  The counts are literal: a change of the host code that adds, drops or swaps a launch shows up here by name.

``CASES`` / ``run_case`` are also what tools/probe_encoder_train_bits.py hashes."""
import collections
import json
import os
import socket
import sys

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (arch, depth, B, size, training, precision, streamed closing convolution, sync BatchNorm)
CASES = {
    "cnn_train": ("CNN", 2, 3, 16, True, "f16x3", True, False),          # streamed closing convolution, fused activation
    "cnn_train_padded": ("CNN", 2, 3, 16, True, "f16x3", False, False),  # CO1_STREAMS = False: padded head, nastar_grad_seed_f16
    "cnn_train_f16": ("CNN", 2, 3, 16, True, "f16", True, False),        # plain fp16 operands: no weight maxima
    "downsize_train": ("CNNDownSize", 2, 3, 32, True, "f16x3", True, False),  # pooling: streamed closing convolution, no fusion
    "cnn_evalgrad": ("CNN", 2, 3, 16, False, "f16x3", True, False),      # eval() with gradients: unfused, eval-mode bias gradients
    "downsize_evalgrad": ("CNNDownSize", 2, 3, 32, False, "f16x3", True, False),
    "unet_train": ("Unet", 3, 2, 32, True, "f16x3", True, False),
    "unet_evalgrad": ("Unet", 3, 2, 32, False, "f16x3", True, False),
    "cnn_train_sync": ("CNN", 2, 3, 16, True, "f16x3", True, True),      # SyncBatchNorm forced in a one-rank gloo group
    "unet_train_sync": ("Unet", 3, 2, 32, True, "f16x3", True, True),
}

# counted on the commit before encoder_train.py's BatchNorm steps were written once; every case of CASES, every function called
EXPECTED = {
    "cnn_train": {
        "nastar_absmax_multi_f32": 1, "nastar_bn1_fwd_partial": 1, "nastar_bn1_parts": 2, "nastar_bn1_sigmoid_bwd": 1,
        "nastar_bn1_sigmoid_bwd_partial": 1, "nastar_bn1_sigmoid_fwd": 1, "nastar_bn_stats_coef_bwd_f16": 1,
        "nastar_bn_stats_coef_bwd_u1_f16": 1, "nastar_bn_stats_coef_fwd_f16": 2, "nastar_chan_affine_f16": 2,
        "nastar_chan_affine_u1_f16": 1, "nastar_chan_stats_workspace_bytes": 4, "nastar_conv3x3_co1_f16": 1,
        "nastar_conv3x3_co1_wgrad_f16": 1, "nastar_conv3x3_co1_workspace_bytes": 2, "nastar_conv3x3_f16": 3,
        "nastar_conv3x3_wgrad_f16": 2, "nastar_conv3x3_wgrad_workspace_bytes": 2, "nastar_encoder_prep_f16": 1,
        "nastar_grad_scale_f32": 1, "nastar_pack_conv_weights_multi_f16": 1,
    },
    "cnn_train_padded": {
        "nastar_absmax_multi_f32": 1, "nastar_bn1_fwd_partial": 1, "nastar_bn1_parts": 2, "nastar_bn1_sigmoid_bwd": 1,
        "nastar_bn1_sigmoid_bwd_partial": 1, "nastar_bn1_sigmoid_fwd": 1, "nastar_bn_stats_coef_bwd_f16": 2,
        "nastar_bn_stats_coef_fwd_f16": 2, "nastar_chan_affine_f16": 4, "nastar_chan_stats_workspace_bytes": 4,
        "nastar_conv3x3_f16": 5, "nastar_conv3x3_wgrad_f16": 3, "nastar_conv3x3_wgrad_workspace_bytes": 3,
        "nastar_encoder_prep_f16": 1, "nastar_grad_seed_f16": 1, "nastar_pack_conv_weights_multi_f16": 1,
    },
    "cnn_train_f16": {
        "nastar_bn1_fwd_partial": 1, "nastar_bn1_parts": 2, "nastar_bn1_sigmoid_bwd": 1, "nastar_bn1_sigmoid_bwd_partial": 1,
        "nastar_bn1_sigmoid_fwd": 1, "nastar_bn_stats_coef_bwd_f16": 1, "nastar_bn_stats_coef_bwd_u1_f16": 1,
        "nastar_bn_stats_coef_fwd_f16": 2, "nastar_chan_affine_f16": 2, "nastar_chan_affine_u1_f16": 1,
        "nastar_chan_stats_workspace_bytes": 4, "nastar_conv3x3_co1_f16": 1, "nastar_conv3x3_co1_wgrad_f16": 1,
        "nastar_conv3x3_co1_workspace_bytes": 2, "nastar_conv3x3_f16": 3, "nastar_conv3x3_wgrad_f16": 2,
        "nastar_conv3x3_wgrad_workspace_bytes": 2, "nastar_encoder_prep_f16": 1, "nastar_grad_scale_f32": 1,
        "nastar_pack_conv_weights_multi_f16": 1,
    },
    "downsize_train": {
        "nastar_absmax_multi_f32": 1, "nastar_bn1_fwd_partial": 1, "nastar_bn1_parts": 2, "nastar_bn1_sigmoid_bwd": 1,
        "nastar_bn1_sigmoid_bwd_partial": 1, "nastar_bn1_sigmoid_fwd": 1, "nastar_bn_stats_coef_bwd_f16": 2,
        "nastar_bn_stats_coef_fwd_f16": 2, "nastar_chan_affine_f16": 4, "nastar_chan_stats_workspace_bytes": 4,
        "nastar_conv3x3_co1_f16": 1, "nastar_conv3x3_co1_workspace_bytes": 1, "nastar_conv3x3_f16": 4,
        "nastar_conv3x3_wgrad_f16": 3, "nastar_conv3x3_wgrad_workspace_bytes": 3, "nastar_encoder_prep_f16": 1, "nastar_grad_seed_f16": 1,
        "nastar_maxpool2x2_bwd_f16": 2, "nastar_maxpool2x2_f16": 2, "nastar_pack_conv_weights_multi_f16": 1,
    },
    "cnn_evalgrad": {
        "nastar_absmax_multi_f32": 1, "nastar_bn1_parts": 2, "nastar_bn1_sigmoid_bwd": 1, "nastar_bn1_sigmoid_bwd_partial": 1,
        "nastar_bn1_sigmoid_fwd": 1, "nastar_bn_coef_bwd": 1, "nastar_bn_coef_bwd_io": 1, "nastar_chan_affine_f16": 2,
        "nastar_chan_affine_u1_f16": 1, "nastar_chan_stats_f16_ws": 1, "nastar_chan_stats_u1_f16_ws": 1,
        "nastar_chan_stats_workspace_bytes": 2, "nastar_conv3x3_co1_f16": 1, "nastar_conv3x3_co1_wgrad_f16": 1,
        "nastar_conv3x3_co1_workspace_bytes": 2, "nastar_conv3x3_f16": 3, "nastar_conv3x3_wgrad_f16": 2,
        "nastar_conv3x3_wgrad_workspace_bytes": 2, "nastar_encoder_prep_f16": 1, "nastar_grad_scale_f32": 1,
        "nastar_pack_conv_weights_multi_f16": 1,
    },
    "downsize_evalgrad": {
        "nastar_absmax_multi_f32": 1, "nastar_bn1_parts": 2, "nastar_bn1_sigmoid_bwd": 1, "nastar_bn1_sigmoid_bwd_partial": 1,
        "nastar_bn1_sigmoid_fwd": 1, "nastar_bn_coef_bwd": 2, "nastar_chan_affine_f16": 4, "nastar_chan_stats_f16_ws": 2,
        "nastar_chan_stats_workspace_bytes": 2, "nastar_conv3x3_co1_f16": 1, "nastar_conv3x3_co1_workspace_bytes": 1,
        "nastar_conv3x3_f16": 4, "nastar_conv3x3_wgrad_f16": 3, "nastar_conv3x3_wgrad_workspace_bytes": 3,
        "nastar_encoder_prep_f16": 1, "nastar_grad_seed_f16": 1, "nastar_maxpool2x2_bwd_f16": 2, "nastar_maxpool2x2_f16": 2,
        "nastar_pack_conv_weights_multi_f16": 1,
    },
    "unet_train": {
        "nastar_absmax_multi_f32": 1, "nastar_bn_stats_coef_bwd_f16": 18, "nastar_bn_stats_coef_fwd_f16": 18,
        "nastar_chan_affine_f16": 36, "nastar_chan_stats_workspace_bytes": 36, "nastar_conv3x3_f16": 37,
        "nastar_conv3x3_wgrad_f16": 19, "nastar_conv3x3_wgrad_workspace_bytes": 19, "nastar_encoder_prep_f16": 1, "nastar_grad_add_f16": 2,
        "nastar_grad_seed_f16": 1, "nastar_maxpool2x2_bwd_f16": 3, "nastar_maxpool2x2_f16": 3,
        "nastar_pack_conv_weights_multi_f16": 1, "nastar_upcat_bwd_f16": 3, "nastar_upcat_f16": 3,
    },
    "unet_evalgrad": {
        "nastar_absmax_multi_f32": 1, "nastar_bn_coef_bwd_io": 18, "nastar_chan_affine_f16": 36, "nastar_chan_stats_f16_ws": 18,
        "nastar_chan_stats_workspace_bytes": 18, "nastar_conv3x3_f16": 37, "nastar_conv3x3_wgrad_f16": 19,
        "nastar_conv3x3_wgrad_workspace_bytes": 19, "nastar_encoder_prep_f16": 1, "nastar_grad_add_f16": 2,
        "nastar_grad_seed_f16": 1, "nastar_maxpool2x2_bwd_f16": 3, "nastar_maxpool2x2_f16": 3, "nastar_pack_conv_weights_multi_f16": 1,
        "nastar_upcat_bwd_f16": 3, "nastar_upcat_f16": 3,
    },
    "cnn_train_sync": {
        "nastar_absmax_multi_f32": 1, "nastar_bn1_fwd_partial": 1, "nastar_bn1_parts": 2, "nastar_bn1_sigmoid_bwd": 1,
        "nastar_bn1_sigmoid_bwd_partial": 1, "nastar_bn1_sigmoid_fwd": 1, "nastar_bn_coef_bwd": 1, "nastar_bn_coef_bwd_io": 1,
        "nastar_bn_coef_fwd": 2, "nastar_chan_affine_f16": 2, "nastar_chan_affine_u1_f16": 1, "nastar_chan_stats_f16_ws": 3,
        "nastar_chan_stats_u1_f16_ws": 1, "nastar_chan_stats_workspace_bytes": 4, "nastar_conv3x3_co1_f16": 1,
        "nastar_conv3x3_co1_wgrad_f16": 1, "nastar_conv3x3_co1_workspace_bytes": 2, "nastar_conv3x3_f16": 3,
        "nastar_conv3x3_wgrad_f16": 2, "nastar_conv3x3_wgrad_workspace_bytes": 2, "nastar_encoder_prep_f16": 1,
        "nastar_grad_scale_f32": 1, "nastar_pack_conv_weights_multi_f16": 1,
    },
    "unet_train_sync": {
        "nastar_absmax_multi_f32": 1, "nastar_bn_coef_bwd_io": 18, "nastar_bn_coef_fwd": 18, "nastar_chan_affine_f16": 36,
        "nastar_chan_stats_f16_ws": 36, "nastar_chan_stats_workspace_bytes": 36, "nastar_conv3x3_f16": 37,
        "nastar_conv3x3_wgrad_f16": 19, "nastar_conv3x3_wgrad_workspace_bytes": 19, "nastar_encoder_prep_f16": 1,
        "nastar_grad_add_f16": 2, "nastar_grad_seed_f16": 1, "nastar_maxpool2x2_bwd_f16": 3, "nastar_maxpool2x2_f16": 3,
        "nastar_pack_conv_weights_multi_f16": 1, "nastar_upcat_bwd_f16": 3, "nastar_upcat_f16": 3,
    },
}


class _Recorder:
    """the real library behind a proxy that notes the name of every ``nastar_*`` function called, then calls through"""

    def __init__(self, lib, names):
        self._lib, self._names = lib, names

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("nastar_"):
            return fn

        def call(*args):
            self._names.append(name)
            return fn(*args)
        return call


def record_launches():
    """replace ``encoder_train._native.load`` by the recording proxy: (names list, restore())"""
    from neural_astar import encoder_train as ET
    real = ET._native.load
    names = []
    proxy = _Recorder(real(), names)
    ET._native.load = lambda: proxy

    def restore():
        ET._native.load = real
    return names, restore


def run_case(name, dev):
    """one ``encode`` + ``backward`` of CASES[name] from fixed seeds: (planner, cost map)"""
    from neural_astar import encoder_train as ET
    from neural_astar.planner import NeuralAstar
    from neural_astar.utils import synthetic as syn
    arch, depth, B, size, training, precision, co1, _sync = CASES[name]
    torch.manual_seed(17 + depth)
    na = NeuralAstar(encoder_input="m+", encoder_arch=arch, encoder_depth=depth, const=3.0)
    g = torch.Generator().manual_seed(size + B)
    with torch.no_grad():
        for mod in na.encoder.modules():
            if isinstance(mod, nn.BatchNorm2d):  # running statistics that are not the batch's, an affine part that is not the identity
                mod.weight.copy_(torch.rand(mod.weight.shape, generator=g) + 0.5)
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.2)
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.3)
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) * 1.5 + 0.5)
    na = na.to(dev).train(training)
    na.encoder_backend = "hip_" + precision
    pr = syn.random_obstacle_maps(B, size, size, 0.25, seed=5)
    m, s, gl = (torch.from_numpy(x).to(dev) for x in pr)
    out = size >> depth if arch == "CNNDownSize" else size
    R = torch.randn((B, 1, out, out), generator=g) / (B * out * out)
    keep = ET.CO1_STREAMS
    try:
        ET.CO1_STREAMS = co1
        cost = na.encode(m, s, gl)
        kind = "train" if training else "evalgrad"
        assert na.last_encoder_route == f"hip:{arch}-{kind}/{precision}", na.last_encoder_route
        (cost * R.to(dev)).sum().backward()
    finally:
        ET.CO1_STREAMS = keep
    torch.cuda.synchronize()
    return na, cost


def sync_worker(rank, port, out_dir, names, job):
    """child process: the sync cases ``names`` under SyncBatchNorm forced in a one-rank gloo group; ``job(name, planner, cost,
    launches)`` -> a JSON-able result per case, written to ``out_dir``/sync.json"""
    import torch.distributed as dist
    sys.path[:0] = [os.path.join(ROOT, "neural-astar_amd"), ROOT, os.path.join(ROOT, "tests")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=0, world_size=1)
    from neural_astar import encoder_train as ET
    ET.SyncBatchNorm.enabled = ET.SyncBatchNorm.force = True
    res = {}
    for name in names:
        launches, restore = record_launches()
        try:
            na, cost = run_case(name, dev)
        finally:
            restore()
        res[name] = job(name, na, cost, launches)
    json.dump(res, open(os.path.join(out_dir, "sync.json"), "w"))
    dist.destroy_process_group()


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _counts(name, na, cost, launches):
    return dict(collections.Counter(launches))


@pytest.fixture
def launches():
    names, restore = record_launches()
    yield names
    restore()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, c in CASES.items() if not c[7]])
def test_launches_of_one_training_step(name, launches):
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    run_case(name, torch.device("cuda:0"))
    got = dict(collections.Counter(launches))
    print("LAUNCHES", name, json.dumps(got, sort_keys=True))
    assert got == EXPECTED[name]


@pytest.mark.gpu
def test_launches_of_one_training_step_sync_batchnorm(tmp_path):
    """the statistics -> all-reduce -> coefficients form of every hidden BatchNorm, forward and backward (CNN and U-Net)"""
    import torch.multiprocessing as mp
    names = [n for n, c in CASES.items() if c[7]]
    mp.spawn(sync_worker, args=(free_port(), str(tmp_path), names, _counts), nprocs=1, join=True)
    got = json.load(open(tmp_path / "sync.json"))
    print("LAUNCHES", json.dumps(got, sort_keys=True))
    for name in names:
        assert got[name] == EXPECTED[name], name

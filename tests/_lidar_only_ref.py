"""What the four-feature tests share (tests/test_lidar_only_host.py, tests/test_gpu_lidar_only.py).  Not a test module; imports
torch, the oracle and `synthetic`, never the library.

  * init_state_dict(F, seed): default-initialised weights of the reference architecture over F point features, in the reference's
    construction order (model/point_net2.py:77-99: MLP1 = [F + 3, 16, 16], MLP1_fp = [34 + F, 34]) with its state-dict keys -- the
    oracle's `network.init_state_dict` with the two widths that depend on F.  F = 8 gives that function's numbers.
  * lidar_batch(B, N, first_plot): a `synthetic.make_batch` batch twice -- `six`: the cloud's rows `synthetic.LIDAR_ROWS`
    (x, y, z, intensity, return_num, num_returns: what a four-feature model reads, and what the oracle is run on); `ten`: the same
    plots as a ten-row cloud whose colour rows 3..6 are NaN, so that any kernel that touched them would show.
  * train_ref / eval_ref: the oracle's fp64 training step (oracle/check.py: train_step) and eval forward on the six-row cloud,
    computed once per argument tuple and never modified.
"""
import functools
from collections import OrderedDict

import torch

from oracle import check, network
from stratanet2_vegetation_coverage_maps_amd.synthetic import LIDAR_ROWS, make_args, make_batch

COLOUR_ROWS = (3, 4, 5, 6)


def layers(F):
    """(prefix, [channel sizes]) in the construction order of model/point_net2.py:81-96 with n_input_feats = F."""
    out = OrderedDict(network.LAYERS)
    out["sa1_module.conv.local_nn"] = [F + 3, 16, 16]
    out["fp1_module.nn"] = [34 + F, 34]
    return out


def init_state_dict(F, seed=0):
    torch.manual_seed(seed)
    sd = OrderedDict()
    for prefix, ch in layers(F).items():
        for i in range(1, len(ch)):
            lin = torch.nn.Linear(ch[i - 1], ch[i])
            bn = torch.nn.BatchNorm1d(ch[i])
            for k, v in lin.state_dict().items():
                sd[f"{prefix}.{i - 1}.0.{k}"] = v.detach().clone()
            for k, v in bn.state_dict().items():
                sd[f"{prefix}.{i - 1}.2.{k}"] = v.detach().clone()
    lin1 = torch.nn.Linear(34, 16)
    lin2 = torch.nn.Linear(16, 5)
    sd["lin1.weight"], sd["lin1.bias"] = lin1.weight.detach().clone(), lin1.bias.detach().clone()
    sd["lin2.weight"] = lin2.weight.detach().clone()
    sd["lin2.bias"] = torch.tensor(network.LIN2_BIAS)
    return sd


def lidar_args(N, ratio1, r1=1.0, r2=2.0, **kw):
    return make_args(subsample_size=N, n_input_feats=6, ratio1=ratio1, r1=r1, ratio2=0.25, r2=r2, **kw)


def fps_start(B, N):
    return torch.stack([torch.arange(B) * 7 % N, torch.arange(B) * 3 % 50])


@functools.lru_cache(maxsize=None)
def lidar_batch(B, N, first_plot=300):
    """-> (six, ten): two `cloud_data` dicts over the same plots (shared xyz, coverages, pdf_all, fps_start)."""
    d = make_batch(B, N, first_plot=first_plot)
    d["fps_start"] = fps_start(B, N)
    six, ten = dict(d), dict(d)
    six["cloud"] = d["cloud"][:, list(LIDAR_ROWS)].contiguous()
    ten["cloud"] = d["cloud"].clone()
    ten["cloud"][:, list(COLOUR_ROWS)] = float("nan")
    return six, ten


def with_running_statistics(sd, seed):
    """A state dict whose BatchNorms carry running statistics that are not the batch's (as after some epochs of training)."""
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict((k, v.clone()) for k, v in sd.items())
    for k in sd:
        if k.endswith("running_mean"):
            sd[k] = 0.2 * torch.randn(sd[k].shape, generator=g)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(sd[k].shape, generator=g)
        elif k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(7)
    return sd


def state_dict_for(seed, training=True):
    """The weights of a step: default initialisation; an eval-mode step (training=False) also gets running statistics."""
    sd = init_state_dict(4, seed)
    return sd if training else with_running_statistics(sd, seed + 100)


@functools.lru_cache(maxsize=None)
def train_ref(B, N, ratio1, seed, use_kdtree=False, training=True, bf16=False, first_plot=300):
    """The oracle's step on the six-row cloud: fp64 (the yardstick); bf16: the same with the operands of `BF16_BLOCKS`' layers rounded to bfloat16."""
    from stratanet2_vegetation_coverage_maps_amd import PointNet2
    six, _ = lidar_batch(B, N, first_plot)
    kw = dict(bf16_layers=PointNet2.BF16_BLOCKS) if bf16 else {}
    return check.train_step(state_dict_for(seed, training), six, lidar_args(N, ratio1), fps_start=six["fps_start"], use_kdtree=use_kdtree,
                            training=training, **kw)


def eval_ref(sd_now, B, N, ratio1, first_plot=300):
    """The oracle's eval forward (fp32, as tests/test_gpu_network.py compares it) on the six-row cloud with the given state."""
    six, _ = lidar_batch(B, N, first_plot)
    with torch.no_grad():
        cov, proba, _ = network.forward(sd_now, six["cloud"], six["xyz"], lidar_args(N, ratio1), training=False,
                                        fps_start=(six["fps_start"][0], six["fps_start"][1]), use_kdtree=True)
    return cov, proba

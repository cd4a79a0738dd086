"""The "3sa-arch" variant BASELINE.json's configuration 2 names -- three ball-query set-abstraction levels (npoint
1024 / 256 / 64, radius 1 / 2 / 4 m) before the global one -- on the same kernels ("make the stack generic so a
third ball-query level (npoint 64, r = 4.0, MLP[35,64]) can precede the global pool (then FP4 k=1, FP3/2/1 k=3)").

THE REFERENCE HAS NO SUCH MODEL (`model/point_net2.py:84-96` builds two ball-query levels + the global one): this class is
for throughput measurements next to the reference architecture; its parity partner is the oracle's generalisation
(`oracle/network.py::forward_3sa`), not the reference.

    SA1 [11,16,16] -> SA2 [19,32] -> SA3 [35,64] (ball query, ratio3, r3) -> SA4 global [67,64] -> max
    FP4 k=1 [64+64,64] -> FP3 k=3 [64+32,64] -> FP2 k=3 [64+16,34] -> FP1 k=3 [34+8,34] -> head (as the reference)

This file only DESCRIBES the architecture: the modules and a few settings.  Every pass -- geometry (single and grouped), forward,
backward, their buffers and descriptors -- is `PointNet2`'s per-call path, which is written over the number of ball-query levels
it finds (`PointNet2.sa_levels`); handles and saved sets number their attributes by level (idx3, knn4, h_sa4, x4, arg4, ...).

`cloud_data["n_live"]` (PointNet2's additive key: the plots' live prefixes for the FPS kernels) is IGNORED here: the three FPS
levels of this variant always sample over all points, and `TrainPipeline` does not hand the key on (`geometry_takes_n_live`).
"""
import torch
from torch import nn

from .point_net2 import MLP, FPModule, GlobalSAModule, PointNet2, SAModule


class PointNet2ThreeSA(PointNet2):
    def __init__(self, args):
        nn.Module.__init__(self)
        self._init_fields(args)
        self.sa1_module = SAModule(args.ratio1, args.r1, MLP([11, 16, 16]))
        self.sa2_module = SAModule(args.ratio2, args.r2, MLP([19, 32]))
        self.sa3_module = SAModule(getattr(args, "ratio3", 0.25), getattr(args, "r3", 4.0), MLP([35, 64]))
        self.sa4_module = GlobalSAModule(MLP([67, 64]))
        self.fp4_module = FPModule(1, MLP([64 + 64, 64]))
        self.fp3_module = FPModule(3, MLP([64 + 32, 64]))
        self.fp2_module = FPModule(3, MLP([64 + 16, 34]))
        self.fp1_module = FPModule(3, MLP([34 + 8, 34]))
        self.lin1 = nn.Linear(34, 16)
        self.lin2 = nn.Linear(16, self.n_class + 1)
        self.lin2.bias = nn.Parameter(torch.tensor([0.733, 0.266, 0.235, 0.358, 0.500]))
        self.softmax = nn.Softmax(dim=1)
        self.sigmoid = nn.Sigmoid()
        if self.cuda_device is not None:
            self.cuda(self.cuda_device)

    BF16_BLOCKS = ("sa1_module.conv.local_nn", "sa2_module.conv.local_nn", "sa3_module.conv.local_nn", "sa4_module.nn",
                   "fp4_module.nn", "fp3_module.nn", "fp2_module.nn")
    SUPPORTED_FEATS = (8,)          # MLP([11, 16, 16]) and MLP([34 + 8, 34]) above are written for the reference's eight point features
    executor = False                # the one-call C executor (csrc/net.hip) covers the reference architecture only
    geometry_fork = False           # its geometry passes run on one stream: forking them is a change that needs a measurement
    # the one-launch global-level kernels are written for 35 -> 64 and 96 -> 64; their route rules ask about B, rows and bf16
    # only, not about widths: this variant's 67 -> 64 and 128 -> 64 must never reach them
    fuse_global_level = False
    fuse_eval_head = False          # eval mode keeps separate FP1 and head launches
    geometry_takes_n_live = False   # cloud_data["n_live"] is ignored (module docstring)

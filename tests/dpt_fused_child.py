"""One forward_window on the forked head path (captured graph) and one on the batched head path (no graph), medium config at 64 x 96:
what tests/test_dpt_fused_gpu.py compares between CUT3R_DPT_FUSE=1 (in its own process) and CUT3R_DPT_FUSE=0 (this module as a child
process: `python -m tests.dpt_fused_child OUT.pt`; Cut3rModel reads the switch when it is built)."""
import os
import sys

import torch

from cut3r_slam_amd.config import Cut3rConfig
from cut3r_slam_amd.model import Cut3rModel
from cut3r_slam_amd.weights import synth_state_dict

DEV = "cuda:0"
KEYS = ("pts3d_in_self_view", "conf_self")


def run(expect_fused):
    cfg = Cut3rConfig(img_size=(64, 96), enc_embed_dim=256, enc_depth=2, enc_num_heads=4, dec_embed_dim=192, dec_depth=3, dec_num_heads=3,
                      state_dec_num_heads=4, state_size=30, local_mem_size=16, ray_enc_depth=1, head_type="dpt", rgb_head=True)
    sd = synth_state_dict(cfg, 5)
    g = torch.Generator().manual_seed(1)
    imgs = torch.randint(0, 256, (4, 3, 64, 96), generator=g, dtype=torch.uint8).to(DEV)
    out = {}
    for path, graphs in (("forked", True), ("batched", False)):
        model = Cut3rModel(cfg, sd, DEV, minimal=True)
        assert model._dpt_fused("downstream_head.dpt_self") == expect_fused, (model.dpt_fuse, expect_fused)
        model.use_graphs = graphs
        preds, _ = model.forward_window(imgs)
        torch.cuda.synchronize()
        # (the forked path exists only inside a capture with the head overlap on: make sure this run took it)
        assert (model._head_stream is not None) == graphs, path
        for k in KEYS:
            t = torch.stack([p[k] for p in preds]).cpu()
            assert bool(torch.isfinite(t).all()), (path, k)
            out[f"{path}.{k}"] = t
        del model
    return out


if __name__ == "__main__":
    fused = os.environ.get("CUT3R_DPT_FUSE", "1") != "0"
    res = run(expect_fused=fused)
    torch.save(res, sys.argv[1])
    print(f"dpt_fused_child: fused={fused}, {len(res)} tensors saved")

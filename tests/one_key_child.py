"""What tests/test_one_key_model_gpu.py compares between CUT3R_ONE_KEY=1 and CUT3R_ONE_KEY=0, each in a fresh process (`python -m
tests.one_key_child OUT.pt`; Cut3rModel reads its switches from the environment when it is built): the tiny and the 768-wide
configuration of profiles/decoder_refactor/summary.md, minimal True and False, `forward_window(return_taps=True)` (every prediction, every
state tap and every memory tap) and `decode_windows` (3 windows of 3 views)."""
import os
import sys

import torch

from cut3r_slam_amd.config import Cut3rConfig
from cut3r_slam_amd.model import Cut3rModel
from cut3r_slam_amd.weights import synth_state_dict

DEV = "cuda:0"
H, W = 64, 96
CONFIGS = {
    "tiny": (Cut3rConfig(img_size=(H, W), enc_embed_dim=256, enc_depth=2, enc_num_heads=4, dec_embed_dim=192, dec_depth=4, dec_num_heads=3,
                         state_dec_num_heads=4, state_size=30, local_mem_size=16, ray_enc_depth=1, head_type="dpt", rgb_head=True), 5),
    "wide": (Cut3rConfig(img_size=(H, W), enc_embed_dim=256, enc_depth=1, enc_num_heads=4, dec_embed_dim=768, dec_depth=2, dec_num_heads=12,
                         state_dec_num_heads=16, state_size=30, local_mem_size=16, ray_enc_depth=1, head_type="dpt", rgb_head=True), 7),
}


def run():
    one_key = os.environ.get("CUT3R_ONE_KEY", "1") != "0"
    g = torch.Generator().manual_seed(1)
    imgs = torch.randint(0, 256, (9, 3, H, W), generator=g, dtype=torch.uint8).to(DEV)
    out = {}
    for name, (cfg, seed) in CONFIGS.items():
        sd = synth_state_dict(cfg, seed)
        for minimal in (True, False):
            model = Cut3rModel(cfg, sd, DEV, minimal=minimal)
            assert model.one_key == one_key
            tag = f"{name}.{'minimal' if minimal else 'full'}"
            preds, taps = model.forward_window(imgs[:3], return_taps=True)
            for i, p in enumerate(preds):
                for k, v in p.items():
                    out[f"{tag}.window.view{i}.{k}"] = v.cpu()
            for i, (st, mem) in enumerate(taps["states"]):
                out[f"{tag}.window.state{i}"], out[f"{tag}.window.mem{i}"] = st.cpu(), mem.cpu()
            feats = model.encode_batch(imgs)
            res = model.decode_windows(feats.view(3, 3, *feats.shape[1:]), H, W)
            for k, v in res.items():
                out[f"{tag}.windows.{k}"] = v.cpu()
            torch.cuda.synchronize()
            del model
    for k, v in out.items():
        assert bool(torch.isfinite(v).all()), k
    return out


if __name__ == "__main__":
    res = run()
    torch.save(res, sys.argv[1])
    print(f"one_key_child: CUT3R_ONE_KEY={os.environ.get('CUT3R_ONE_KEY', '1')}, {len(res)} tensors saved")

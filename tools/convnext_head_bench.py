"""Forward + backward of the ConvNeXt semantic-segmentation head alone (ConvNeXtAdapter, bf16) at the ADE20K (B = 4, 512 x 512,
150 classes) and NYUv2 (B = 2, 640 x 640, 40 classes) geometries of cfgs/finetune/semseg/ (embed_dim 6144, preds_per_patch 16,
depth 4, ViT-B tokens), beside a plain-torch restatement of the same head on the same GPU (channels-last, bf16 autocast) as the
yardstick.  Writes profiles/convnext_head_bench.json.

    python tools/convnext_head_bench.py [--iters 20] [--out profiles/convnext_head_bench.json]

Per-kernel times come from a separate run under the kernel tracer (rocprofv3 --kernel-trace --stats -d out -- python
tools/convnext_head_bench.py --iters 5 --only engine), whose stats table is copied to profiles/convnext_head_kernel_stats.csv.
"""
import argparse
import json
import math
import os
import sys

import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import multimae_amd as M  # noqa: E402
from multimae_amd import output_adapters as OA  # noqa: E402

GEOMS = {'ade20k': dict(B=4, H=512, W=512, K=150), 'nyuv2': dict(B=2, H=640, W=640, K=40)}
D, E, P, DEPTH = 768, 6144, 16, 4


class TorchHead(nn.Module):
    """the yardstick: the same head in plain torch, channels-last map, depthwise conv through cuDNN/MIOpen, bf16 autocast"""

    def __init__(self, K):
        super().__init__()
        C = E // P
        self.proj_dec = nn.Linear(D, E)
        self.blocks = nn.ModuleList(nn.ModuleDict(dict(dwconv=nn.Conv2d(C, C, 7, padding=3, groups=C), norm=nn.LayerNorm(C, eps=1e-6),
                                                       pwconv1=nn.Linear(C, 4 * C), pwconv2=nn.Linear(4 * C, C))) for _ in range(DEPTH))
        self.final_layer = nn.Conv2d(C, K, 1)

    def forward(self, x, H, W):
        B, s, C = x.shape[0], int(math.isqrt(P)), E // P
        NH, NW = H // 16, W // 16
        z = self.proj_dec(x[:, :NH * NW])
        z = z.view(B, NH, NW, s, s, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, NH * s, NW * s).contiguous(memory_format=torch.channels_last)
        for b in self.blocks:
            t = b['dwconv'](z).permute(0, 2, 3, 1)
            t = b['pwconv2'](F.gelu(b['pwconv1'](b['norm'](t))))
            z = z + t.permute(0, 3, 1, 2)
        z = self.final_layer(z)
        return F.interpolate(z.float(), size=(H, W), mode='bilinear', align_corners=False)


def _time(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--only', choices=['engine', 'torch', 'both'], default='both')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'convnext_head_bench.json'))
    a = ap.parse_args()
    res = {'device': torch.cuda.get_device_name(), 'iters': a.iters, 'precision': 'bf16', 'geometries': {}}
    for name, g in GEOMS.items():
        B, H, W, K = g['B'], g['H'], g['W'], g['K']
        N = (H // 16) * (W // 16)
        torch.manual_seed(0)
        x = (torch.randn(B, N + 1, D, device='cuda') * 0.5).requires_grad_(True)
        gout = torch.randn(B, K, H, W, device='cuda')
        row = dict(g)
        if a.only in ('engine', 'both'):
            head = OA.ConvNeXtAdapter(num_classes=K, embed_dim=E, preds_per_patch=P, depth=DEPTH)
            head.init(D)
            head = head.cuda()
            info = {'tasks': {'rgb': {'start_idx': 0, 'end_idx': N, 'num_tokens': N}}, 'image_size': (H, W)}

            def eng():
                y = head(x, info)
                y.backward(gout)
            with M.engine.precision('bf16'):
                row['engine_ms'] = _time(eng, a.iters)
                row['engine_fwd_ms'] = _time(lambda: head(x.detach(), info), a.iters)
            del head
        if a.only in ('torch', 'both'):
            th = TorchHead(K).cuda().to(memory_format=torch.channels_last)

            def tor():
                with torch.autocast('cuda', dtype=torch.bfloat16):
                    y = th(x, H, W)
                y.backward(gout)
            row['torch_ms'] = _time(tor, a.iters)
            with torch.no_grad():
                def torf():
                    with torch.autocast('cuda', dtype=torch.bfloat16):
                        th(x, H, W)
                row['torch_fwd_ms'] = _time(torf, a.iters)
            del th
        C, h, w = E // P, (H // 16) * 4, (W // 16) * 4
        row['map_bytes_f32'] = B * h * w * C * 4
        row['dwconv_fwd_compulsory_bytes'] = 2 * row['map_bytes_f32']          # read x, write y
        row['dwconv_dgrad_compulsory_bytes'] = 3 * row['map_bytes_f32']        # read dy, read dx_in, write dx
        row['resize_fwd_compulsory_bytes'] = B * K * H * W * 4 + B * h * w * K * 4
        res['geometries'][name] = row
        print(name, json.dumps(row), flush=True)
        torch.cuda.empty_cache()
    if a.only == 'both':
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()

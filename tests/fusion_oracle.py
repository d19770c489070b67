"""The tests' own torch restatement of the RefineNet pieces of the DPT head (output_adapter_utils.py:60-247) as plain functions of a
state dict: F.conv2d / F.relu / F.interpolate, nothing else.  tests/test_fusion_blocks_cpu.py checks that it reproduces the
reference's recorded f32 outputs and gradients (tests/golden/fusion_blocks.npz) bit for bit, so the GPU tests may use it at shapes
the fixture does not hold; in f64 it is the reference the element-wise bounds are taken against."""
import torch
import torch.nn.functional as F


def conv3x3(x, w, b=None, stride=1):
    return F.conv2d(x, w, b, stride=stride, padding=1)


def rcu(x, sd, pre=''):
    """ResidualConvUnit_custom: conv2(relu(conv1(relu(x)))) + x"""
    out = conv3x3(F.relu(x), sd[pre + 'conv1.weight'], sd[pre + 'conv1.bias'])
    out = conv3x3(F.relu(out), sd[pre + 'conv2.weight'], sd[pre + 'conv2.bias'])
    return out + x


def upsample2x(x):
    return F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=True)


def fusion(xs, sd, pre=''):
    """FeatureFusionBlock_custom with one or two inputs"""
    out = xs[0]
    if len(xs) == 2:
        out = out + rcu(xs[1], sd, pre + 'resConfUnit1.')
    out = rcu(out, sd, pre + 'resConfUnit2.')
    return F.conv2d(upsample2x(out), sd[pre + 'out_conv.weight'], sd[pre + 'out_conv.bias'])


def weight_like(y):
    """the fixed output weighting of the backward checks (tests/golden/make_golden_fusion.py)"""
    return torch.sin(0.37 * torch.arange(y.numel(), dtype=torch.float64)).to(y.dtype).view(y.shape).to(y.device)


def run(fn, xs, sd, dtype=torch.float32):
    """forward + backward of fn(xs..., sd) with the sin weighting: (y, [dx], {name: grad}) on the CPU in `dtype`"""
    sd = {k: v.detach().to('cpu', dtype).clone().requires_grad_(True) for k, v in sd.items()}
    xs = [x.detach().to('cpu', dtype).clone().requires_grad_(True) for x in xs]
    y = fn(xs, sd) if fn is fusion else fn(xs[0], sd)
    (y * weight_like(y)).sum().backward()
    return y.detach(), [x.grad for x in xs], {k: v.grad for k, v in sd.items() if v.grad is not None}

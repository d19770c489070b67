"""GPU: the kernels on the heads' low-resolution map (resize, regression losses, depth metrics, segmentation loss and argmax) and the
soft-target cross-entropy return the bits tests/golden/lowres_bits.npz recorded from the build before their index map, gather walk
and fixed-order sums were written once (csrc/resize_map.h, common.h).  tests/golden/make_lowres_bits.py lists the cases."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import make_lowres_bits as LB  # noqa: E402


def test_lowres_kernels_keep_the_bits_of_the_build_before_the_shared_map_and_sums():
    z = np.load(LB.PATH)
    index, flat = LB.pack(LB.run({k[3:]: z[k] for k in z.files if k.startswith('in_')}))
    assert index == json.loads(str(z['out_index']))
    gold = {d: torch.from_numpy(z['out_' + d]) for d in flat}
    off, bad = dict.fromkeys(flat, 0), []
    for name, d, shape in index:
        part = slice(off[d], off[d] + math.prod(shape))
        off[d] = part.stop
        assert flat[d].dtype == gold[d].dtype
        if not torch.equal(flat[d][part], gold[d][part]):                # int32 (f32), int16 (bf16) and int64 views: the bits
            bad.append((name, int((flat[d][part] != gold[d][part]).sum())))
    assert not bad and all(off[d] == gold[d].numel() for d in flat), bad

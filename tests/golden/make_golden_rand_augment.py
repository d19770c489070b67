"""Golden fixture for RandAugment from the reference's own ``utils/auto_augment.py`` run on PIL images.  The file is loaded by path, so
that ``utils/__init__.py``'s other imports are not needed.

``rand_augment.npz``:
  meta                 JSON: PIL version, the fill colour, the op cases and the policy cases (below)
  img/<name>           the input images, uint8 (3, H, W): ``r24x40`` seeded noise, ``r8x8`` seeded noise (64 pixels: Equalize's step is
                       0), ``c8x8`` one colour (AutoContrast's hi <= lo, Equalize's single bin), ``p<k>`` the policy inputs (16 x 24)
  (a) op cases         meta['ops']: a list of {id, image, name, magnitude, negate, interp, fn, args}: the reference's level function of
                       ``name`` at ``magnitude`` (``_randomly_negate`` forced to ``negate``), then its image function ``fn`` with the
                       resulting ``args`` (and ``resample=interp``, ``fillcolor=fill`` for the geometric ones).  Each of the 15
                       increasing ops and the 6 names that differ in the non-increasing list, at magnitudes 0, 5 and 10, both signs
                       where the level function negates, bicubic and bilinear where it resamples.
  op_small[slot]       the output bytes of the cases on the 8 x 8 images (``slot`` is in the case)
  op_digest[slot]      for ``r24x40`` the SHA-256 digest of the output bytes (32 bytes): the noise image's outputs do not
                       compress, and some 330 KB of them would not fit a committed fixture.  A digest
                       pins every byte all the same; ``tests/test_rand_augment_cpu.py`` also compares the restatement with PIL itself
                       in full where PIL is importable.
  (b) policy cases     meta['policies']: {config, hparams, seed, images, applied, random, np_rand}: after ``random.seed(seed);
                       np.random.seed(seed)`` the policy is called on the 8 images in a row.  ``applied[k]`` lists what ran on image
                       k: [chosen name, fn, args, interp] per op that passed ``prob`` (fn None for one that did not), ``random`` /
                       ``np_rand`` are the next ``random.random()`` / ``np.random.rand()`` after the run.
  policy_out[i][k]     the output bytes of image k under policy case i

The generator fails when its cases lose one of: an Equalize with step == 0; an AutoContrast channel with hi <= lo; a blend factor above 1
that clips; a geometric op that leaves fill pixels; a stats-needing op (AutoContrast, Equalize, Contrast) applied as the second op of
a sample after a first op that changed the image.

Build container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rand_augment.py
"""
import hashlib
import importlib.util
import json
import os
import random
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF  # noqa: E402

OUT = os.path.join(HERE, 'rand_augment.npz')
FILL = (124, 116, 104)                       # round(255 * IMAGENET_DEFAULT_MEAN)
INCREASING = ['AutoContrast', 'Equalize', 'Invert', 'Rotate', 'PosterizeIncreasing', 'SolarizeIncreasing', 'SolarizeAdd',
              'ColorIncreasing', 'ContrastIncreasing', 'BrightnessIncreasing', 'SharpnessIncreasing', 'ShearX', 'ShearY',
              'TranslateXRel', 'TranslateYRel']
PLAIN = ['Posterize', 'Solarize', 'Color', 'Contrast', 'Brightness', 'Sharpness']
GEOMETRIC = ('Rotate', 'ShearX', 'ShearY', 'TranslateXRel', 'TranslateYRel')
NEGATES = GEOMETRIC + ('ColorIncreasing', 'ContrastIncreasing', 'BrightnessIncreasing', 'SharpnessIncreasing')
STATS = ('auto_contrast', 'equalize', 'contrast')
POLICIES = [dict(config='rand-m9-mstd0.5-inc1', hparams=dict(translate_const=100, img_mean=FILL, interpolation=Image.BICUBIC), seed=11),
            dict(config='rand-m9-mstd0.5-inc1', hparams=dict(translate_const=100, img_mean=FILL), seed=12),       # random interpolation
            dict(config='rand-m7-n3-w0', hparams=dict(translate_const=100, img_mean=FILL, interpolation=Image.BILINEAR), seed=13)]


def load_reference():
    spec = importlib.util.spec_from_file_location('ref_auto_augment', os.path.join(REF, 'utils', 'auto_augment.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def to_pil(a):
    return Image.fromarray(np.ascontiguousarray(a.transpose(1, 2, 0)))


def to_chw(im):
    return np.ascontiguousarray(np.asarray(im).transpose(2, 0, 1))


def images():
    rng = np.random.RandomState(20240)
    img = {'r24x40': rng.randint(0, 256, (3, 24, 40)).astype(np.uint8), 'r8x8': rng.randint(0, 256, (3, 8, 8)).astype(np.uint8)}
    img['c8x8'] = np.broadcast_to(np.array([17, 200, 96], dtype=np.uint8)[:, None, None], (3, 8, 8)).copy()
    for k in range(8):
        p = rng.randint(0, 256, (3, 16, 24)).astype(np.uint8)
        if k % 2:                                                   # narrow ranges: AutoContrast and Equalize have something to do
            p = (60 + p // 3).astype(np.uint8)
        img[f'p{k}'] = p
    return img


def main():
    ref = load_reference()
    img = images()
    out = {f'img/{k}': v for k, v in img.items()}
    seen = dict(eq_step0=False, ac_flat=False, blend_clip=False, fill_left=False, stats_second=False)
    fill = np.array(FILL, dtype=np.uint8)[:, None, None]

    # ---- (a) every op, called directly ---------------------------------------------------------------------------------------------
    ops, digests, small = [], [], []
    sign = [False]
    ref._randomly_negate = lambda v: -v if sign[0] else v
    hparams = dict(translate_const=100, img_mean=FILL)
    for name in INCREASING + PLAIN:
        level_fn, fn = ref.LEVEL_TO_ARG[name], ref.NAME_TO_OP[name]
        mags = (0., 5., 10.) if level_fn is not None else (0.,)
        for mag in mags:
            for neg in ((False, True) if name in NEGATES else (False,)):
                for interp in ((Image.BICUBIC, Image.BILINEAR) if name in GEOMETRIC else (0,)):
                    sign[0] = neg
                    args = level_fn(mag, hparams) if level_fn is not None else ()
                    kwargs = dict(resample=int(interp), fillcolor=FILL) if name in GEOMETRIC else {}
                    for iname in ('r24x40', 'r8x8', 'c8x8'):
                        y = to_chw(fn(to_pil(img[iname]), *args, **dict(kwargs)))
                        case = dict(id=len(ops), image=iname, name=name, magnitude=mag, negate=neg, interp=int(interp),
                                    fn=fn.__name__, args=[float(a) if isinstance(a, float) else int(a) for a in args])
                        ops.append(case)
                        store = digests if iname == 'r24x40' else small
                        case['slot'] = len(store)
                        store.append(np.frombuffer(hashlib.sha256(y.tobytes()).digest(), dtype=np.uint8) if iname == 'r24x40' else y)
                        x = img[iname]
                        if fn.__name__ == 'equalize' and iname == 'r8x8':
                            seen['eq_step0'] |= (x.shape[1] * x.shape[2] - 1) // 255 == 0 and np.array_equal(x, y)
                        if fn.__name__ == 'auto_contrast' and iname == 'c8x8':
                            seen['ac_flat'] |= np.array_equal(x, y)
                        if fn.__name__ == 'brightness' and args[0] > 1:
                            seen['blend_clip'] |= bool(((y == 255) & (x < 255) & (x * float(args[0]) > 256)).any())
                        if name in GEOMETRIC and mag > 0:
                            seen['fill_left'] |= bool(np.all(y == fill, axis=0).any())

    # ---- (b) whole policies ----------------------------------------------------------------------------------------------------------
    log = []
    for fname, fn in list(ref.NAME_TO_OP.items()):
        def wrapped(im, *args, _fn=fn, **kwargs):
            log.append(dict(fn=_fn.__name__, args=[float(a) if isinstance(a, float) else int(a) for a in args], interp=0, before=to_chw(im)))
            res = _fn(im, *args, **kwargs)
            log[-1]['after'] = to_chw(res)
            return res
        ref.NAME_TO_OP[fname] = wrapped
    interpolation = ref._interpolation

    def logged_interpolation(kwargs):
        r = interpolation(kwargs)
        log[-1]['interp'] = int(r)
        return r
    ref._interpolation = logged_interpolation
    ref._randomly_negate = lambda v: -v if random.random() > 0.5 else v          # the reference's own again
    calls = []
    op_call = ref.AugmentOp.__call__

    def logged_call(self, im):
        n0 = len(log)
        res = op_call(self, im)
        assert len(log) - n0 in (0, 1)
        calls.append([names[id(self)]] + ([log[-1]['fn'], log[-1]['args'], log[-1]['interp']] if len(log) > n0 else [None, [], 0]))
        return res
    ref.AugmentOp.__call__ = logged_call
    policies, outputs = [], []
    for i, pc in enumerate(POLICIES):
        tf = ref.rand_augment_transform(pc['config'], dict(pc['hparams']))
        names = {id(op): n for op, n in zip(tf.ops, INCREASING if 'inc' in pc['config'] else ref._RAND_TRANSFORMS)}
        choice = np.random.choice
        picked = []

        def logged_choice(a, *args, **kw):
            r = choice(a, *args, **kw)
            picked.append([names[id(op)] for op in r])
            return r
        ref.np.random.choice = logged_choice
        random.seed(pc['seed'])
        np.random.seed(pc['seed'])
        applied = []
        try:
            for k in range(8):
                del log[:]
                del calls[:]
                y = to_chw(tf(to_pil(img[f'p{k}'])))
                outputs.append(y)
                ran = list(calls)
                assert [r[0] for r in ran] == picked[-1]
                applied.append(ran)
                if len(log) >= 2 and log[1]['fn'] in STATS and not np.array_equal(log[0]['before'], log[0]['after']) \
                        and not np.array_equal(log[1]['before'], log[1]['after']):
                    seen['stats_second'] = True
        finally:
            ref.np.random.choice = choice
        hp = {k: (list(v) if isinstance(v, tuple) else int(v)) for k, v in pc['hparams'].items()}
        policies.append(dict(config=pc['config'], hparams=hp, seed=pc['seed'], images=[f'p{k}' for k in range(8)], applied=applied,
                             random=random.random(), np_rand=float(np.random.rand())))
        print(pc['config'], pc['seed'], [[r[1] for r in a] for a in applied])
    assert all(seen.values()), f'the cases no longer cover {[k for k, v in seen.items() if not v]}'
    out['op_digest'], out['op_small'] = np.stack(digests), np.stack(small)
    out['policy_out'] = np.stack(outputs).reshape(len(POLICIES), 8, *outputs[0].shape)
    out['meta'] = np.array(json.dumps(dict(pil=PIL.__version__, fill=list(FILL), ops=ops, policies=policies)))
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes,', len(ops), 'op cases')


if __name__ == '__main__':
    main()

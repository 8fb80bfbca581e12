#!/usr/bin/env python3
"""What the reference's own utils/image.py (scipy.ndimage.affine_transform underneath) makes of the augmentation test inputs
(tests/_augment_cases.make_inputs): its matrices, its float64 output of affine_cv, its uint8 cast, its outside masks, and the parameters and
first-image result of one seeded call of its rand_aff_noisy_cv.  Prints the table of digests that tests/_augment_cases.REFERENCE records
(paste it there when the inputs change); --out FILE.npz also keeps the arrays, for inspection.  CPU only; needs the reference tree and scipy.

No file of reference results is committed: tests/golden/ has to hold exactly what oracle/gen_golden.py writes (tools/check_golden_regen.py),
so the tests carry digests, rebuild the inputs from their seed, and tests/test_augment_model.py calls generate() where the reference tree is
present to compare the float64 values and to re-derive the digests.

The reference module is imported in place.  Shims on this side only: stub modules for what it imports and this tool never calls (cv2,
and torchvision / PIL where absent), and a module-level `map` that returns a list (np.dstack(map(...)) needs a sequence on Python 3).

Usage: python tools/gen_augment_golden.py [--reference DIR] [--out FILE.npz]"""
import argparse
import builtins
import importlib.util
import os
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _augment_cases as cases  # noqa: E402

SHAPES, SEED = cases.SHAPES, cases.SEED


def load_reference(ref_dir):
    for name in ("cv2", "torchvision", "torchvision.transforms", "PIL", "PIL.Image"):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    cv2 = sys.modules["cv2"]
    if not hasattr(cv2, "INTER_CUBIC"):
        cv2.INTER_CUBIC = 2
    for parent, child in (("torchvision", "transforms"), ("PIL", "Image")):
        if not hasattr(sys.modules[parent], child):
            setattr(sys.modules[parent], child, sys.modules[parent + "." + child])
    spec = importlib.util.spec_from_file_location("_reference_utils_image", os.path.join(ref_dir, "utils", "image.py"))
    mod = importlib.util.module_from_spec(spec)
    mod.map = lambda f, *its: list(builtins.map(f, *its))
    spec.loader.exec_module(mod)
    return mod


def generate(ref_dir):
    ref = load_reference(ref_dir)
    seen = []
    real = ref.interpolation.affine_transform

    def recording(channel, m, offset, **kw):
        seen.append(np.concatenate([np.asarray(m)[0], [offset[0]], np.asarray(m)[1], [offset[1]]]))
        return real(channel, m, offset, **kw)

    out = dict(cases.make_inputs())
    ref.interpolation.affine_transform = recording
    try:
        for s, (n, H, W) in enumerate(SHAPES):
            imgs, params = out["img%d" % s], out["params%d" % s]
            f64, mats = [], []
            for i in range(n):
                del seen[:]
                f64.append(ref.affine_cv(imgs[i].astype(float), *params[i], cval=.1))
                mats.append(seen[0])
            f64 = np.stack(f64)
            out["mat%d" % s], out["f64_%d" % s], out["u8_%d" % s] = np.stack(mats), f64, f64.astype(np.uint8)
            out["outside%d" % s] = (f64 == .1).all(-1)
        # one seeded call of the reference's own closure: pins the order in which it draws its parameters
        seen_params = []
        real_affine = ref.affine_cv

        def spy(img, angle, v_shift, h_shift, sx, sy, cval=0.):
            seen_params.append((angle, v_shift, h_shift, sx, sy))
            return real_affine(img, angle, v_shift, h_shift, sx, sy, cval=cval)

        ref.affine_cv = spy
        np.random.seed(SEED)
        random.seed(SEED)
        first = ref.random_affine_noisy_cv(rotation=45, hs_range=.25, vs_range=.25, h_flip=True, h_range=.05, v_range=.1)(out["img0"][0])
        out["draw_params"], out["draw_u8"] = np.array(seen_params[0]), first
        out["draw_outside"] = (real_affine(out["img0"][0].astype(float), *seen_params[0], cval=.1) == .1).all(-1)
    finally:
        ref.interpolation.affine_transform = real
    return out


def digest_table(data):
    n = len(SHAPES)
    return cases.table([data["mat%d" % s] for s in range(n)], [data["outside%d" % s] for s in range(n)], [data["u8_%d" % s] for s in range(n)],
                       data["draw_params"], data["draw_outside"], data["draw_u8"])


def main():
    import pprint
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("ISX_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=None, help="also write the arrays to this .npz (not a committed file)")
    a = ap.parse_args()
    data = generate(a.reference)
    if a.out:
        np.savez_compressed(a.out, **data)
    print("REFERENCE = " + pprint.pformat(digest_table(data), width=140, sort_dicts=True))


if __name__ == "__main__":
    main()

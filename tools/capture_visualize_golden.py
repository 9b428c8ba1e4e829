"""Capture tests/golden/visualize_ref.npz: tiny random inputs and the FLOAT outputs of the reference's utils/visualize.py on them
(make_example_img(resize_factor=None), make_test_img, make_test_detailed_img, pred_to_colormap), which tests/test_visualize_cpu.py
and the GPU tests quantise with plt.imsave's rule, floor(x * 255).

    python tools/capture_visualize_golden.py --reference /path/to/VQ_SEG [--out tests/golden/visualize_ref.npz]

The reference imports cv2 at module top; the functions captured here never call it, so a stand-in module object takes its place.
pred_to_detailed_colormap counts the classes as len(np.unique(target)) and accepts only 3, so the targets cover all three classes.
Not a test; nothing that runs on the GPU imports this file.  Only the data it writes belongs to the repository.
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

B, C, H, W = 2, 3, 6, 10
DETAIL_COLORMAP = [[0, 0, 0], [0, 0, 1], [1, 0, 0], [0.5, 0.5, 0.5], [230 / 255, 145 / 255, 56 / 255], [1, 217 / 255, 102 / 255]]   # test_detailviz.py:129


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="root of the reference source tree (holds utils/visualize.py)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "visualize_ref.npz"))
    args = ap.parse_args()
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    spec = importlib.util.spec_from_file_location("reference_visualize", os.path.join(args.reference, "utils", "visualize.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    rng = np.random.default_rng(20240)
    l_input, ul_input = (rng.random((B, 3, H, W), dtype=np.float32) for _ in range(2))
    pred, ul_pred = ((rng.standard_normal((B, C, H, W)) * 4).astype(np.float32) for _ in range(2))
    target = rng.integers(0, C, (B, H, W)).astype(np.int64)
    target[:, 0, :C] = np.arange(C)                          # every image holds every class
    cm = np.array(DETAIL_COLORMAP, dtype=np.float64)
    v1, v2 = ref.make_test_img(l_input, pred.copy(), target)
    d1, d2 = ref.make_test_detailed_img(l_input, pred.copy(), target, colormap=cm)
    np.savez_compressed(
        args.out, l_input=l_input, ul_input=ul_input, pred=pred, ul_pred=ul_pred, target=target, detail_colormap=cm,
        example=ref.make_example_img(l_input, target, pred.copy(), ul_input, ul_pred.copy(), resize_factor=None),
        example_labelled=ref.make_example_img(l_input, target, pred.copy(), None, None),
        test_v1=v1, test_v2=v2, detail_v1=d1, detail_v2=d2,
        pred_colormap=ref.pred_to_colormap(pred.copy(), cm[:C]))
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()

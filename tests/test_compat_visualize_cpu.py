"""The last two lines of the reference trainer's import block (train_vqreptunet1x1v2.py:18-19) bind through `<repo>/compat`:
`from utils.processing import detach_numpy` and `from utils.visualize import make_example_img, save_img`.  A fresh interpreter
whose sys.path holds nothing else of this repository, from a foreign working directory (as tests/test_compat_cpu.py).  `import utils`
imports every submodule of vq_seg_amd.utils, so none of them may pull in matplotlib, PIL or cv2."""
import json
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = textwrap.dedent('''
    import json, sys
    sys.path.insert(0, sys.argv[1])                 # the ONE line a maintainer adds: <repo>/compat
    import utils
    heavy = [m for m in ("matplotlib", "PIL", "cv2") if m in sys.modules]
    from utils.processing import detach_numpy
    from utils.visualize import make_example_img, save_img
    import numpy as np
    import torch
    import vq_seg_amd.utils.processing, vq_seg_amd.utils.visualize
    t = torch.arange(6.0, requires_grad=True).reshape(2, 3)
    a = detach_numpy(t * 2)
    rng = np.random.default_rng(0)
    sheet = make_example_img(rng.random((2, 3, 4, 6), dtype=np.float32), rng.integers(0, 3, (2, 4, 6)), rng.standard_normal((2, 3, 4, 6)),
                             rng.random((2, 3, 4, 6), dtype=np.float32), rng.standard_normal((2, 3, 4, 6)))
    print(json.dumps({
        "heavy": heavy,
        "same": [detach_numpy is vq_seg_amd.utils.processing.detach_numpy, make_example_img is vq_seg_amd.utils.visualize.make_example_img,
                 save_img is vq_seg_amd.utils.visualize.save_img, utils.visualize is vq_seg_amd.utils.visualize],
        "numpy": [type(a).__name__, a.tolist()],
        "sheet": [list(sheet.shape), str(sheet.dtype)],
        "after": [m for m in ("matplotlib", "cv2") if m in sys.modules]}))
''')


def test_reference_trainer_visualize_imports_bind(tmp_path):
    script = tmp_path / "trainer_head.py"
    script.write_text(SCRIPT)
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    res = subprocess.run([sys.executable, str(script), os.path.join(ROOT, "compat")], cwd=str(tmp_path), env=env, capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["heavy"] == []                                    # `import utils` pulled in none of matplotlib, PIL, cv2
    assert out["same"] == [True, True, True, True]
    assert out["numpy"] == ["ndarray", [[0.0, 2.0, 4.0], [6.0, 8.0, 10.0]]]
    assert out["sheet"] == [[4, 22, 3], "uint8"]                 # (2 * 4 / 2, (4 * 6 + 20) / 2, 3): the reference's default resize_factor
    assert out["after"] == []                                    # composing a sheet needs neither

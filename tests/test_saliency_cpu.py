"""RBD saliency without a GPU: the float64 restatement of tests/saliency_cases.py against networkx and against its own linear system, the
torch-op form of vq_seg_amd.utils.saliency against the restatement, salient_masking against the reference's formula
(deprecated/train_salient.py:29-34, restated with index assignment), CPSConfig's validation and the reference's entry points through
`compat`."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import saliency_cases as sal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(sal.CASES)


def _torch_parts(name, dtype):
    from vq_seg_amd.utils.saliency import saliency_rbd_from_labels_torch
    lab, labels, grid = sal.make(name)
    out, parts = saliency_rbd_from_labels_torch(torch.from_numpy(lab.copy()).to(dtype), torch.from_numpy(labels.copy()), grid, return_parts=True)
    return out, parts


@pytest.mark.parametrize("name", NAMES)
def test_restated_geodesic_is_dijkstra(name):
    nx = pytest.importorskip("networkx")
    ref = sal.reference(name)
    wgt, geo = ref["weights"], ref["geodesic"]
    for n in range(wgt.shape[0]):
        graph = nx.Graph()
        graph.add_nodes_from(range(wgt.shape[1]))
        for i, j in zip(*np.nonzero(np.isfinite(wgt[n]) & ~np.eye(wgt.shape[1], dtype=bool))):
            graph.add_edge(int(i), int(j), weight=float(wgt[n, i, j]))
        want = np.full(wgt[n].shape, np.inf)
        for i, row in nx.all_pairs_dijkstra_path_length(graph, weight="weight"):
            for j, d in row.items():
                want[i, j] = d
        assert np.array_equal(np.isinf(want), np.isinf(geo[n]))
        fin = np.isfinite(want)
        assert (np.abs(geo[n][fin] - want[fin]) <= 1e-12 * np.maximum(want[fin], 1.0)).all()
        act = ref["stats"][n, :, 5] > 0
        assert np.isfinite(geo[n][np.ix_(act, act)]).all()      # the active clusters of a covering map are connected


@pytest.mark.parametrize("name", NAMES)
def test_restated_solve_satisfies_the_system(name):
    ref = sal.reference(name)
    for n, (a, rhs, ix, _wn) in enumerate(sal.system64(ref["geodesic"], ref["stats"], ref["adj"], ref["w_bg"], ref["wctr"])):
        assert np.array_equal(a, a.T) and np.linalg.eigvalsh(a).min() > 0.0
        x = ref["x"][n, ix]
        assert np.abs(a @ x - rhs).max() <= 1e-12 * max(1.0, np.abs(rhs).max())
        assert (ref["x"][n, np.setdiff1d(np.arange(ref["x"].shape[1]), ix)] == 0).all()
    assert ref["sal"].min() >= 0.0 and ref["sal"].max() <= 1.0


def test_the_cases_are_what_they_claim():
    ref = sal.reference("blobs_emptied")
    assert ref["stats"][0, 19, 5] == 0 and (ref["stats"][1:, :, 5] > 0).all()            # one cluster emptied, in image 0 only
    assert (sal.reference("all_boundary")["stats"][..., 6] == 1).all()
    assert sal.CASES["k144_ragged_tiles"][2] * sal.CASES["k144_ragged_tiles"][3] == 144
    const = sal.reference("constant")
    act = const["stats"][0, :, 5] > 0
    assert (const["geodesic"][0][np.ix_(act, act)] == 0).all() and (const["sal"] == 0).all()
    for name in NAMES:
        if name != "constant":
            r = sal.reference(name)
            assert r["sal"].max() == 1.0 and r["sal"].min() == 0.0, name


@pytest.mark.parametrize("name", NAMES)
def test_torch_form_float64_equals_the_restatement(name):
    ref = sal.reference(name)
    out, parts = _torch_parts(name, torch.float64)
    assert out.dtype == torch.float64
    assert np.array_equal(parts["adj"].numpy(), ref["adj"])
    assert np.array_equal(parts["stats"][..., 5:7].numpy(), ref["stats"][..., 5:7])
    assert np.array_equal(np.isinf(parts["geodesic"].numpy()), np.isinf(ref["geodesic"]))
    for key in ("stats", "geodesic", "w_bg", "wctr", "wctr_norm", "x", "xnorm"):
        got, want = parts[key].numpy(), ref[key]
        fin = np.isfinite(want)
        err = np.abs(got[fin] - want[fin]).max()
        assert err <= 1e-10 * max(1.0, np.abs(want[fin]).max()), (key, err)
    assert np.abs(out.numpy() - ref["sal"]).max() <= 1e-10


@pytest.mark.parametrize("name", NAMES)
def test_torch_form_float32_is_finite(name):
    out, parts = _torch_parts(name, torch.float32)
    assert out.dtype == torch.float32 and bool(torch.isfinite(out).all()) and float(out.min()) >= 0.0 and float(out.max()) <= 1.0
    for key in ("w_bg", "wctr", "wctr_norm", "x", "xnorm"):
        assert bool(torch.isfinite(parts[key]).all()), key
    if name == "constant":
        assert not bool(out.any())


def test_public_functions_on_cpu_tensors():
    from vq_seg_amd import utils
    from vq_seg_amd.utils import saliency
    assert utils.saliency_rbd is saliency.saliency_rbd and utils.salient_masking is saliency.salient_masking
    assert utils.saliency_rbd_from_labels is saliency.saliency_rbd_from_labels
    images = torch.rand(2, 3, 40, 48, generator=torch.Generator().manual_seed(3))
    images[:, :, 10:30, 12:36] = images[:, :, 10:30, 12:36] * 0.2 + torch.tensor([0.7, 0.1, 0.1])[None, :, None, None]
    out, parts = saliency.saliency_rbd(images, 30, return_parts=True)
    assert out.shape == (2, 40, 48) and out.dtype == torch.float32 and float(out.min()) == 0.0 and float(out.max()) == 1.0
    assert saliency.saliency_rbd(images.double(), 30).dtype == torch.float64
    lab, labels, grid = sal.make("noise")
    got = saliency.saliency_rbd_from_labels(torch.from_numpy(lab.copy()), torch.from_numpy(labels.copy()), grid)
    assert np.abs(got.numpy() - sal.reference("noise")["sal"]).max() <= 1e-4
    with pytest.raises(ValueError):
        saliency.saliency_rbd(images[0])
    with pytest.raises(ValueError):
        saliency.saliency_rbd(images, 30, sigma_clr=0.0)
    with pytest.raises(ValueError):
        saliency.saliency_rbd_from_labels(torch.from_numpy(lab.copy()), torch.from_numpy(labels.copy()).float(), grid)


def test_a_label_outside_its_window_is_ignored():
    from vq_seg_amd.utils.saliency import saliency_rbd_from_labels_torch
    lab, labels, (gy, gx) = sal.make("noise")
    bad = labels.copy()
    bad[0, 0, 0], bad[0, 5, 5], bad[1, 3, 3] = gy * gx - 1, -7, 10 ** 6          # far from home, negative, past the table
    want = sal.rbd64(lab, bad, gy, gx)
    assert want["sal"][0, 0, 0] == 0 and want["sal"][0, 5, 5] == 0 and want["sal"][1, 3, 3] == 0
    got = saliency_rbd_from_labels_torch(torch.from_numpy(lab.copy()).double(), torch.from_numpy(bad), (gy, gx))
    assert np.abs(got.numpy() - want["sal"]).max() <= 1e-10


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16])
def test_salient_masking_is_the_references_formula(dtype):
    from vq_seg_amd.utils.saliency import salient_masking
    gen = torch.Generator().manual_seed(11)
    pred = torch.randn(2, 3, 9, 7, generator=gen).to(dtype)
    sal_map = torch.rand(2, 9, 7, generator=gen)
    sal_map[0, 0, 0], sal_map[1, 2, 3] = 0.1, 0.0                               # the threshold itself counts as background

    def reference(p, s):                                                        # train_salient.py:29-34
        bg_n, bg_y, bg_x = (s <= 0.1).nonzero(as_tuple=True)
        mask = torch.ones_like(p, dtype=torch.float)
        mask[bg_n, 1, bg_y, bg_x] = 0
        mask[bg_n, 2, bg_y, bg_x] = 0
        return p * mask

    a, b = pred.clone().requires_grad_(True), pred.clone().requires_grad_(True)
    got, want = salient_masking(a, sal_map, 0.1), reference(b, sal_map)
    assert got.dtype == dtype and torch.equal(got.float(), want.float())
    assert torch.equal(got[:, 0], pred[:, 0]) and bool((got[0, 1:, 0, 0] == 0).all())
    weight = torch.randn(2, 3, 9, 7, generator=gen)
    (got.float() * weight).sum().backward()
    (want.float() * weight).sum().backward()
    assert torch.equal(a.grad, b.grad) and bool((a.grad[0, 1:, 0, 0] == 0).all())
    with pytest.raises(ValueError):
        salient_masking(pred, sal_map[:1])
    with pytest.raises(ValueError):
        salient_masking(pred.long(), sal_map)


def test_config_validation():
    from vq_seg_amd.trainer import CPSConfig as Config
    model = {"name": "vqreptunet1x1", "params": {"encoder_name": "resnet50", "num_classes": 3, "depth": 5,
                                                 "vq_cfg": {"num_embeddings": [0, 0, 64, 64, 64], "distance": "euclidean", "kmeans_init": True},
                                                 "margin": 0.0, "scale": 1.0, "use_feature": False, "encoder_weights": None}}
    CPSConfig = lambda **kw: Config(model=model, **kw)                          # noqa: E731
    assert CPSConfig().salient_mask is None and CPSConfig().salient_segments == 250
    assert CPSConfig(salient_mask=0.1, salient_segments=64).salient_mask == 0.1
    assert CPSConfig(recipe="v2", salient_mask=0.0, superpixel_mean=36).salient_mask == 0.0
    for bad in (dict(salient_mask=-0.1), dict(salient_mask=1.0), dict(salient_mask=True), dict(salient_segments=0),
                dict(salient_segments=1025), dict(salient_segments=2.5), dict(salient_segments=True)):
        with pytest.raises(ValueError):
            CPSConfig(**bad)


def test_refusals_without_a_gpu():
    """the entry points refuse bad shapes before anything touches a device, and nnf.saliency_rbd has no CPU form"""
    from vq_seg_amd import _hip, nnf
    L = _hip.lib()
    assert L.vqseg_region_graph_f(None, None, 1, 64, 64, 8, 8, None, None, None) == -1 and b"null" in L.vqseg_last_error()
    assert L.vqseg_rbd_geodesic_f(None, 1, 8, None) == -1 and b"null" in L.vqseg_last_error()
    with pytest.raises(_hip.HipLibraryError, match="at most 1024 superpixels"):
        nnf.saliency_rbd(torch.zeros(1, 3, 128, 128), 1100)
    with pytest.raises(_hip.HipLibraryError, match="float32"):
        nnf.saliency_rbd(torch.zeros(1, 3, 32, 32, dtype=torch.float64), 16)
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        nnf.saliency_rbd(torch.zeros(1, 3, 32, 32), 16)
    with pytest.raises(_hip.HipLibraryError, match="int32"):
        nnf.rbd_from_labels(torch.zeros(1, 3, 32, 32), torch.zeros(1, 32, 32, dtype=torch.int64), (4, 4))
    assert not nnf.rbd_supported(torch.zeros(1, 3, 32, 32)) and nnf.RBD_MAX_SEGMENTS == 1024


def test_compat_entry_points_in_a_fresh_interpreter(tmp_path):
    code = (
        "import sys, numpy as np\n"
        f"sys.path.insert(0, {os.path.join(ROOT, 'compat')!r})\n"
        "from saliency_map import get_saliency_rbd\n"
        "from saliency_map.saliency import get_saliency_ft\n"
        "import vq_seg_amd.utils.saliency as real\n"
        "assert get_saliency_rbd is real.get_saliency_rbd\n"
        "rng = np.random.default_rng(0)\n"
        "img = (rng.uniform(0, 60, (40, 48, 3))).astype(np.uint8)\n"
        "img[10:30, 12:36] = (200, 40, 40)\n"
        "out = get_saliency_rbd(img, n_segments=30)\n"
        "assert out.shape == (40, 48) and out.dtype == np.float64, (out.shape, out.dtype)\n"
        "assert out.min() == 0.0 and out.max() == 255.0, (out.min(), out.max())\n"
        "gray = get_saliency_rbd(img[..., 0], n_segments=30)\n"
        "assert gray.shape == (40, 48) and np.isfinite(gray).all()\n"
        "try:\n"
        "    get_saliency_ft('x.png')\n"
        "except NotImplementedError as e:\n"
        "    assert 'get_saliency_ft' in str(e)\n"
        "else:\n"
        "    raise SystemExit('get_saliency_ft did not raise')\n"
        "print('ok')\n")
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(tmp_path), env=env)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stderr[-2000:]

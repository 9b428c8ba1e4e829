"""DeviceLoader on the GPU: every batch is torch.equal to what the reference's loop gets from DataLoader(BaseDataset) +
img_to_label (train_vqreptunet1x1v2.py:89-90,130-139) -- same files in the same order, same values, same global RNG draws --
and two CPS iterations fed by either loader give bit-identical losses and pseudo-label masks."""
import itertools
import os

import pytest
import torch
from PIL import Image
from torch.utils.data import DataLoader

from vq_seg_amd.data import BaseDataset, DeviceLoader, write_synthetic_dataset
from vq_seg_amd.utils.seg_tools import img_to_label

pytestmark = pytest.mark.gpu

P2L = {"0": 0, "128": 1, "255": 2}
DEV = "cuda:0"


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    r = str(tmp_path_factory.mktemp("crops") / "train")
    write_synthetic_dataset(r, n_labelled=7, n_unlabelled=6, size=(131, 97), seed=9)      # non-square sources, like CWFID's
    return r


def _ref_epoch(loader, mapping):
    out = []
    for b in loader:
        b = dict(b)
        if "target" in b and mapping is not None:
            b["label"] = img_to_label(b["target"], mapping)
        out.append(b)
    return out


def _dev_epoch(loader):
    out = []
    for b in loader:
        assert b["img"].is_cuda and b["img"].is_contiguous(memory_format=torch.channels_last)
        out.append({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in b.items()})
    return out


def _assert_same(ref, got):
    assert len(ref) == len(got)
    for r, g in zip(ref, got):
        assert set(r) == set(g) and r["filename"] == g["filename"]
        for k in ("img", "target", "label"):
            if k in r:
                assert r[k].dtype == g[k].dtype and r[k].shape == g[k].shape and torch.equal(r[k], g[k]), k


def _gen(mode):
    return torch.Generator().manual_seed(1234) if mode == "generator" else None


@pytest.mark.parametrize("split,bs,pad,drop_last,resize,target_resize,shuffle", [
    ("labelled", 4, True, False, 32, True, "off"),             # batch padding (7 -> 8), whole 1 KiB tiles only
    ("labelled", 4, True, False, 32, True, "seed"),            # shuffle under torch.manual_seed
    ("unlabelled", 4, False, True, (40, 24), True, "seed"),    # (w, h) resize, drop_last drops the 6 % 4 tail; partial tiles
    ("unlabelled", 4, False, False, (40, 24), True, "generator"),   # a short last batch, explicit generator
    ("labelled", 3, False, True, None, True, "generator"),     # no resize: 131 x 97 sources (odd sizes: unaligned samples)
    ("labelled", 1, True, False, 32, False, "off"),            # the evaluator's form: 32 x 32 image, 131 x 97 mask
    ("labelled", 2, True, False, 64, True, "seed"),
])
def test_batches_equal_the_reference_loader(root, split, bs, pad, drop_last, resize, target_resize, shuffle):
    ds = BaseDataset(root, split=split, batch_size=bs if pad else None, resize=resize, target_resize=target_resize)
    mapping = P2L if split == "labelled" else None
    kw = dict(batch_size=bs, shuffle=shuffle != "off", drop_last=drop_last)
    torch.manual_seed(321)
    ref_loader = DataLoader(ds, generator=_gen(shuffle), **kw)
    ref = [_ref_epoch(ref_loader, mapping) for _ in range(3)]
    rng_ref = torch.get_rng_state()
    torch.manual_seed(321)
    dl = DeviceLoader(ds, device=DEV, pixel_to_label=mapping, generator=_gen(shuffle), **kw)
    assert len(dl) == len(ref_loader)
    got = [_dev_epoch(dl) for _ in range(3)]
    assert torch.equal(torch.get_rng_state(), rng_ref)
    for r, g in zip(ref, got):
        _assert_same(r, g)
    if shuffle != "off" and len(ref[0]) > 1:
        assert [b["filename"] for b in ref[0]] != [b["filename"] for b in ref[1]] or \
            [b["filename"] for b in ref[1]] != [b["filename"] for b in ref[2]]      # the epochs were really reshuffled
    if split == "labelled":
        assert all("label" in b for b in got[0])


def test_sampler_and_batches_above_one_launch(root):
    """A sampler passed through (here with replacement), and 70-sample batches: more than one launch's argument block (64)."""
    ds = BaseDataset(root, split="labelled", resize=32)

    def sampler():
        return torch.utils.data.RandomSampler(ds, replacement=True, num_samples=140, generator=torch.Generator().manual_seed(8))

    torch.manual_seed(3)
    ref = _ref_epoch(DataLoader(ds, batch_size=70, sampler=sampler()), P2L)
    rng_ref = torch.get_rng_state()
    torch.manual_seed(3)
    got = _dev_epoch(DeviceLoader(ds, batch_size=70, sampler=sampler(), device=DEV, pixel_to_label=P2L))
    assert torch.equal(torch.get_rng_state(), rng_ref) and len(got) == 2 and got[0]["img"].shape == (70, 3, 32, 32)
    _assert_same(ref, got)


def test_zip_cycle_consumes_the_rng_like_the_reference(root):
    """The reference's iteration: zip(itertools.cycle(sup_loader), unsup_loader) with both loaders shuffled (iter() of each
    draws a base seed when it is created, each RandomSampler its permutation seed at the first batch)."""
    sup = BaseDataset(root, split="labelled", batch_size=2, resize=32)
    unsup = BaseDataset(root, split="unlabelled", batch_size=2, resize=32)

    def run(make):
        torch.manual_seed(55)
        s, u = make(sup), make(unsup)
        seq = []
        for _ in range(2):
            for a, b in zip(itertools.cycle(s), u):
                la = img_to_label(a["target"], P2L) if "label" not in a else a["label"]
                seq.append((a["filename"], b["filename"], a["img"].cpu(), la.cpu(), b["img"].cpu()))
        return seq, torch.get_rng_state()

    ref, rng_ref = run(lambda d: DataLoader(d, batch_size=2, shuffle=True))
    got, rng_got = run(lambda d: DeviceLoader(d, batch_size=2, shuffle=True, device=DEV, pixel_to_label=P2L))
    assert torch.equal(rng_ref, rng_got) and len(ref) == len(got) == 6
    for r, g in zip(ref, got):
        assert r[0] == g[0] and r[1] == g[1] and all(torch.equal(x, y) for x, y in zip(r[2:], g[2:]))


def test_every_batch_is_a_fresh_tensor(root):
    dl = DeviceLoader(BaseDataset(root, split="labelled", batch_size=4, resize=32), batch_size=4, device=DEV, pixel_to_label=P2L)
    a, b = list(dl), list(dl)
    ptrs = {t.data_ptr() for batch in a + b for t in (batch["img"], batch["target"], batch["label"])}
    assert len(ptrs) == 3 * len(a + b)
    assert all(torch.equal(x["img"], y["img"]) for x, y in zip(a, b))


def test_mixed_shapes_raise_like_the_default_collate(tmp_path):
    r = str(tmp_path / "mixed")
    write_synthetic_dataset(r, n_labelled=3, n_unlabelled=0, size=(131, 97), seed=2)
    for sub in ("input", "target"):
        p = os.path.join(r, sub, "img_0001.png")
        Image.open(p).resize((64, 48)).save(p)
    ds = BaseDataset(r, split="labelled")
    with pytest.raises(RuntimeError, match="equal size"):
        next(iter(DataLoader(ds, batch_size=3)))
    dl = DeviceLoader(ds, batch_size=3, device=DEV)
    with pytest.raises(RuntimeError, match="equal size"):
        next(iter(dl))
    _assert_same(_ref_epoch(DataLoader(ds, batch_size=1), None), _dev_epoch(DeviceLoader(ds, batch_size=1, device=DEV)))


def test_inputs_the_loader_refuses(root):
    ds = BaseDataset(root, split="labelled", resize=32)
    with pytest.raises(TypeError):
        DeviceLoader(list(range(4)), batch_size=2, device=DEV)
    with pytest.raises(ValueError, match="max_bytes"):
        DeviceLoader(ds, batch_size=2, device=DEV, max_bytes=3 * 32 * 32 * 3)
    dl = DeviceLoader(ds, batch_size=2, device=DEV, max_bytes=7 * (32 * 32 * 3 + 32 * 32))
    assert dl.cache_bytes == 7 * (32 * 32 * 3 + 32 * 32)


def test_cps_iterations_are_bit_identical_to_the_reference_loader(tmp_path):
    """Two CPS iterations at 64 x 64 (v1 recipe, bf16, the benchmark's trainer) driven by zip(cycle(sup), unsup) of either loader:
    every returned loss term and both pseudo-label masks agree bit for bit."""
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer
    r = str(tmp_path / "cps")
    write_synthetic_dataset(r, n_labelled=3, n_unlabelled=4, size=(131, 97), seed=12)
    sup = BaseDataset(r, split="labelled", batch_size=2, resize=64)
    unsup = BaseDataset(r, split="unlabelled", batch_size=2, resize=64)
    dev = torch.device(DEV)
    model = {"name": "vqreptunet1x1", "params": {"encoder_name": "resnet50", "num_classes": 3, "depth": 5,
                                                 "vq_cfg": {"num_embeddings": [0, 0, 64, 64, 64], "distance": "euclidean", "kmeans_init": True},
                                                 "margin": 0.0, "scale": 1.0, "use_feature": False, "encoder_weights": None}}

    def run(device_loader):
        tr = CPSTrainer(CPSConfig(model=model, recipe="v1", total_iters=4, amp_dtype=torch.bfloat16, keep_aux=True), dev)
        torch.manual_seed(2024)
        if device_loader:
            s = DeviceLoader(sup, batch_size=2, shuffle=True, device=dev, pixel_to_label=P2L)
            u = DeviceLoader(unsup, batch_size=2, shuffle=True, device=dev)
        else:
            s, u = DataLoader(sup, batch_size=2, shuffle=True), DataLoader(unsup, batch_size=2, shuffle=True)
        outs = []
        for sup_dict, unsup_dict in zip(itertools.cycle(s), u):
            if device_loader:
                l_in, l_tg, ul = sup_dict["img"], sup_dict["label"], unsup_dict["img"]
            else:                                                   # train_vqreptunet1x1v2.py:130-139
                l_in, ul = sup_dict["img"].to(dev), unsup_dict["img"].to(dev)
                l_tg = img_to_label(sup_dict["target"], P2L).to(dev)
            o = {k: v.detach().cpu().clone() for k, v in tr.step(l_in, l_tg, ul).items()}
            o.update({k: tr.aux[k].detach().cpu().clone() for k in ("mask_1", "mask_2")})
            outs.append(o)
        torch.cuda.synchronize()
        return outs

    ref, got = run(False), run(True)
    assert len(ref) == len(got) == 2
    for a, b in zip(ref, got):
        assert set(a) == set(b)
        assert all(torch.equal(a[k], b[k]) for k in a), {k: (a[k].float().sum(), b[k].float().sum()) for k in a if not torch.equal(a[k], b[k])}

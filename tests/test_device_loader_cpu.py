"""DeviceLoader without a GPU: its two lookup tables are the reference's own ops on every byte value, BaseDataset's split into
_load_u8 + division changes no bit, and the batch-assembly entry point is exported and refuses bad arguments."""
import numpy as np
import pytest
import torch

from vq_seg_amd import _hip
from vq_seg_amd.data import BaseDataset, DeviceLoader, f32_table, label_table, write_synthetic_dataset
from vq_seg_amd.utils.seg_tools import img_to_label

EINVAL = -1


def test_f32_table_is_the_datasets_division():
    t = f32_table()
    assert t.dtype == torch.float32 and t.shape == (256,)
    assert torch.equal(t, torch.arange(256, dtype=torch.uint8).float().div_(255.0))


@pytest.mark.parametrize("mapping", [{"0": 0, "128": 1, "255": 2},          # config/*.json pixel_to_label
                                     {"0": 1, "1": 2, "2": 7, "200": 0}])     # chained: 0 -> 1 -> 2 -> 7, 1 -> 2 -> 7
def test_label_table_is_img_to_label(mapping):
    t = label_table(mapping)
    v = torch.arange(256, dtype=torch.uint8)
    assert t.dtype == torch.int64 and torch.equal(t, img_to_label(v, mapping))
    # as a lookup it reproduces img_to_label on a whole mask batch, unmapped values passing through
    mask = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (2, 17, 9), dtype=np.uint8))
    assert torch.equal(t[mask.long()], img_to_label(mask, mapping))
    if "200" in mapping:
        assert int(t[0]) == 7 and int(t[1]) == 7 and int(t[2]) == 7 and int(t[200]) == 0 and int(t[3]) == 3


@pytest.mark.parametrize("resize,target_resize", [(32, True), ((40, 24), True), (None, True), (32, False)])
def test_load_u8_then_division_is_getitem(tmp_path, resize, target_resize):
    root = str(tmp_path / "d")
    write_synthetic_dataset(root, n_labelled=3, n_unlabelled=2, size=(131, 97), seed=4)
    for split in ("labelled", "unlabelled"):
        ds = BaseDataset(root, split=split, batch_size=2, resize=resize, target_resize=target_resize)
        for i in range(len(ds)):
            img, mask = ds._load_u8(i)
            s = ds[i]
            assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3
            assert torch.equal(img.permute(2, 0, 1).float().div_(255.0), s["img"])
            assert torch.equal(img.permute(2, 0, 1).float() / 255.0, s["img"])
            if split == "labelled":
                assert mask.dtype == torch.uint8 and torch.equal(mask, s["target"])
            else:
                assert mask is None and "target" not in s


def _getitem_before_the_split(ds, index):
    """BaseDataset.__getitem__ as it read before _load_u8 was split out of it, verbatim: pins that the split changed no bit."""
    import os
    from PIL import Image
    filename = ds.filenames[index]
    img = Image.open(os.path.join(ds.img_dir, filename)).convert("RGB")
    target = Image.open(os.path.join(ds.target_dir, filename)).convert("L") if ds.target_dir is not None else None
    if ds.resize is not None:
        img = img.resize(ds.resize, resample=Image.BILINEAR)
        if ds.target_resize and target is not None:
            target = target.resize(ds.resize, resample=Image.NEAREST)
    img = torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).float().div_(255.0)   # TF.to_tensor
    if target is None:
        return {"filename": filename, "img": img}
    return {"filename": filename, "img": img, "target": torch.from_numpy(np.array(target))}


@pytest.mark.parametrize("resize,target_resize", [(32, True), ((40, 24), True), (None, True), (32, False)])
def test_getitem_is_bit_identical_to_before_the_split(tmp_path, resize, target_resize):
    root = str(tmp_path / "d")
    write_synthetic_dataset(root, n_labelled=3, n_unlabelled=2, size=(131, 97), seed=5)
    for split in ("labelled", "unlabelled"):
        ds = BaseDataset(root, split=split, batch_size=2, resize=resize, target_resize=target_resize)
        for i in range(len(ds)):
            old, new = _getitem_before_the_split(ds, i), ds[i]
            assert list(old) == list(new) and old["filename"] == new["filename"]
            for k in ("img", "target"):
                if k in old:
                    assert old[k].dtype == new[k].dtype and old[k].stride() == new[k].stride() and torch.equal(old[k], new[k])


def test_write_synthetic_dataset_non_square(tmp_path):
    from PIL import Image
    root = str(tmp_path / "d")
    write_synthetic_dataset(root, n_labelled=1, n_unlabelled=1, size=(131, 97), seed=1)
    assert Image.open(f"{root}/input/img_0000.png").size == (131, 97)
    assert Image.open(f"{root}/target/img_0000.png").size == (131, 97)


def test_batch_entry_point_rejects_bad_arguments_without_gpu():
    L = _hip.lib()
    assert hasattr(L, "vqseg_batch_u8_f") and "vqseg_batch_u8_f" in _hip.SYMBOLS
    p = 16 * 1024                                   # any non-null address: nothing is dereferenced before validation fails
    off = np.zeros(4, dtype=np.int64)
    offp = off.ctypes.data

    def call(n=4, img=p, mask=None, io=offp, mo=None, h=8, w=8, mh=0, mw=0, f=p, ll=None, out=p, tgt=None, lab=None):
        return L.vqseg_batch_u8_f(n, img, mask, io, mo, h, w, mh, mw, f, ll, out, tgt, lab, None)

    for kw, msg in [(dict(n=0), b"positive"), (dict(h=0), b"positive"), (dict(w=-3), b"positive"),
                    (dict(img=None), b"null"), (dict(io=None), b"null"), (dict(f=None), b"null"), (dict(out=None), b"null"),
                    (dict(mask=p), b"mask cache needs"), (dict(mask=p, mo=offp, tgt=p), b"mask cache needs"),
                    (dict(tgt=p), b"without a mask cache"), (dict(ll=p, lab=p), b"without a mask cache"),
                    (dict(mask=p, mo=offp, mh=8, mw=8, tgt=p, ll=p), b"go together"),
                    (dict(h=1 << 15, w=1 << 14), b"2^28")]:
        assert call(**kw) == EINVAL, kw
        assert msg in L.vqseg_last_error(), (kw, L.vqseg_last_error())
    neg = np.array([0, -16, 0, 0], dtype=np.int64)
    assert call(io=neg.ctypes.data) == EINVAL and b"negative" in L.vqseg_last_error()


def test_wrapper_checks_types_before_the_device():
    cache = torch.zeros(1024, dtype=torch.uint8)
    out = torch.empty((2, 3, 4, 4), dtype=torch.float32).contiguous(memory_format=torch.channels_last)
    with pytest.raises(_hip.HipLibraryError, match="f32_lut"):
        _hip.batch_u8(cache, [0, 64], (4, 4), torch.zeros(256, dtype=torch.float64), out)
    with pytest.raises(_hip.HipLibraryError, match="outside the image cache"):
        _hip.batch_u8(cache, [0, 1000], (4, 4), f32_table(), out)
    with pytest.raises(_hip.HipLibraryError, match="channels_last"):
        _hip.batch_u8(cache, [0, 64], (4, 4), f32_table(), torch.empty((2, 3, 4, 4)))
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        _hip.batch_u8(cache, [0, 64], (4, 4), f32_table(), out)


def test_loader_accepts_only_base_datasets(tmp_path):
    with pytest.raises(TypeError):
        DeviceLoader([{"img": torch.zeros(3, 4, 4)}], batch_size=1)
    with pytest.raises(TypeError):
        DeviceLoader(torch.utils.data.TensorDataset(torch.zeros(4, 3, 2, 2)), batch_size=2)
    root = str(tmp_path / "d")
    write_synthetic_dataset(root, n_labelled=1, n_unlabelled=0, size=16, seed=1)
    with pytest.raises(ValueError, match="no CPU fallback"):
        DeviceLoader(BaseDataset(root, split="labelled"), batch_size=1, device="cpu")

    class Normalised(BaseDataset):                  # its batches would differ from what the cache serves: refused
        def __getitem__(self, index):
            s = super().__getitem__(index)
            s["img"] = (s["img"] - 0.5) / 0.25
            return s

    with pytest.raises(TypeError, match="overrides BaseDataset.__getitem__"):
        DeviceLoader(Normalised(root, split="labelled"), batch_size=1)

    class Renamed(BaseDataset):                     # a subclass that leaves __getitem__ alone passes the type checks
        pass

    with pytest.raises(ValueError, match="no CPU fallback"):
        DeviceLoader(Renamed(root, split="labelled"), batch_size=1, device="cpu")

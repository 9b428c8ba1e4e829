"""The no-grad eval forward of the VQ-UNet (the trainers' pseudo-label pass: split-3 activations, nnf.S3) with its quantised levels
taken by the VQ launch as split-3 rows: against the earlier path (merge to fp32 -> exact kernel -> fp32 gather -> split,
VQSEG_OPTS=py_vq_s3=0) and against the exact kernel merging on load (vq_s3_filter = 0) -- logits and the three levels' code indices
bit for bit.
Reference arithmetic replaced: VectorQuantizer.forward on levels 2-4 of VQRePTUnet1x1.forward (models/networks/modified_vqunet/net.py
of the reference, its eval branch) in the fp32 no-grad forward of train_vqreptunet1x1v2.py:143-149."""
import pytest
import torch

from tests import synth

pytestmark = pytest.mark.gpu


def test_eval_forward_takes_s3_rows_and_matches_the_merged_path(monkeypatch):
    from vq_seg_amd import _hip, nnf
    from vq_seg_amd.models.networks import make_model
    from vq_seg_amd.models.networks.modified_vqunet import net as netmod
    from vq_seg_amd.utils.load_config import AttrDict
    dev = torch.device("cuda:0")
    cfg = AttrDict({"name": "vqreptunet1x1", "params": {
        "encoder_name": "resnet50", "num_classes": 3, "depth": 5,
        "vq_cfg": {"num_embeddings": [0, 0, 256, 256, 256], "distance": "euclidean", "kmeans_init": False},
        "margin": 0.0, "scale": 1.0, "use_feature": False, "encoder_weights": None}})
    torch.manual_seed(0)
    model = make_model(cfg).to(dev)
    model.eval()
    with torch.no_grad():                                     # codes of the features' scale (post-ReLU, sparse), not the tiny uniform init
        for i, vq in enumerate(model.codebook):
            w = getattr(getattr(vq, "codebook", None), "embedding", None)
            if w is not None:
                w.weight.copy_(synth.relu_features(500 + i, tuple(w.weight.shape), sparsity=0.3, scale=1.5))
    x = synth.uniform(21, (2, 3, 64, 64)).to(dev)

    seen = []
    orig = netmod._quantize_group

    def recording(vqs, feats):
        out = orig(vqs, feats)
        seen.append(out)
        return out

    monkeypatch.setattr(netmod, "_quantize_group", recording)

    def run(py_vq_s3, vq_s3_filter):
        seen.clear()
        monkeypatch.setitem(_hip.PY_OPTS, "py_vq_s3", py_vq_s3)
        prev = _hip.set_option("vq_s3_filter", vq_s3_filter)
        before = _hip.set_option("vq_filter_launches", 0)
        try:
            with torch.no_grad():
                logits = model(x)[0]
            torch.cuda.synchronize()
        finally:
            took = _hip.set_option("vq_filter_launches", before)
            _hip.set_option("vq_s3_filter", prev)
        grouped = [o for o in seen if o is not None][-1]
        return logits, [o[1] for o in grouped], isinstance(grouped[0][0], nnf.S3), took

    default = run(1, 1)
    merged = run(0, 1)
    s3_exact = run(1, 0)
    assert default[2] and default[3] == 1, "the default eval forward did not hand split-3 rows to the candidate filter"
    assert not merged[2] and merged[3] == 0
    assert s3_exact[2] and s3_exact[3] == 0
    for other, what in ((merged, "py_vq_s3=0"), (s3_exact, "vq_s3_filter=0")):
        assert torch.equal(default[0], other[0]), f"logits differ from the {what} run"
        for lvl, (a, b) in enumerate(zip(default[1], other[1])):
            assert torch.equal(a, b), f"level {lvl + 2}: indices differ from the {what} run"
    assert len(default[1]) == 3 and default[0].shape == (2, 3, 64, 64) and bool(torch.isfinite(default[0]).all())

"""The non-default stream arms of CPSTrainer.step (the A/B switches of the Python layer and the weight-gradient side
streams) move work between streams and nothing else: every kernel of the path is deterministic, so the parameters after
two steps must equal the default arm's bit for bit -- a difference is a missing stream dependency.

Not among the arms: CPSConfig(wgrad_side_stream=True), alone and with py_stream_prio=1.  Two steps of either end with parameters
that differ from the default arm's in the last digits, the same values run after run and in both: an open finding about the
side-stream arm (profiles/LEDGER.md, "CPSTrainer._step broken up"), not held here until it is understood."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

ARMS = {
    "loss_streams_0": (dict(py_loss_streams=0), {}),
    "opt_streams_0": (dict(py_opt_streams=0), {}),
    "loss_and_opt_streams_0": (dict(py_loss_streams=0, py_opt_streams=0), {}),
    "vq_alone_0": (dict(py_vq_alone=0), {}),
}


def _param_sums(opts, cfg_kw):
    """two steps of the shape of test_trainer_gpu._run (v1, bf16 autocast, 64 x 64, 2 + 2 images); fp64 sum of every parameter"""
    from vq_seg_amd import _hip
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer, SyntheticCropWeed
    dev = torch.device("cuda:0")
    model = {"name": "vqreptunet1x1", "params": {"encoder_name": "resnet50", "num_classes": 3, "depth": 5,
                                                 "vq_cfg": {"num_embeddings": [0, 0, 64, 64, 64], "distance": "euclidean", "kmeans_init": True},
                                                 "margin": 0.0, "scale": 1.0, "use_feature": False, "encoder_weights": None}}
    _hip.lib()                                                   # the library reads VQSEG_OPTS into PY_OPTS when it loads
    _hip.PY_OPTS.update(opts)
    try:
        torch.manual_seed(0)
        tr = CPSTrainer(CPSConfig(model=model, recipe="v1", total_iters=10, amp_dtype=torch.bfloat16, **cfg_kw), dev)
        assert tr._two_streams
        data = SyntheticCropWeed(64, 2, dev, seed=5)
        (l_in, l_tg), ul_in = data.labelled(), data.unlabelled()
        for _ in range(2):
            loss = tr.step(l_in, l_tg, ul_in)["loss"]
        torch.cuda.synchronize()
        assert torch.isfinite(loss).item()
        return torch.stack([p.detach().double().sum() for m in tr.models for p in m.parameters()]).cpu()
    finally:
        for k in opts:
            _hip.PY_OPTS.pop(k, None)


@functools.lru_cache(maxsize=None)
def _default_arm():
    return _param_sums({}, {})


@pytest.mark.parametrize("arm", list(ARMS))
def test_stream_arm_changes_nothing(arm):
    opts, cfg_kw = ARMS[arm]
    assert torch.equal(_param_sums(opts, cfg_kw), _default_arm())

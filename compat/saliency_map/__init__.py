"""`from saliency_map import get_saliency_rbd` / `from saliency_map.saliency import ...` of the reference -> vq_seg_amd.utils.saliency
(see compat/_vqseg_compat.py).  get_saliency_ft is not built and raises NotImplementedError."""
import sys

from _vqseg_compat import bind as _bind

sys.modules[__name__ + ".saliency"] = _bind(__name__, "vq_seg_amd.utils.saliency")

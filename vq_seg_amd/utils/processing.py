"""Tensor -> numpy (reference: utils/processing.py)."""
import torch


def detach_numpy(tensor: torch.Tensor):
    """the tensor's values as a numpy array on the host.  utils.visualize takes device tensors as they are: on the HIP path leave this
    call out in front of make_example_img and only the uint8 sheet crosses to the host."""
    return tensor.detach().cpu().numpy()

"""volume_ssim_layers: the 7 x 7 x 7-window SSIM map of a volume pair, summed layer by layer (C ABI ``afcm_volume_ssim``, include/afcm_hip.h).

One call turns two stacks of volumes into a float64 ``[volumes, d - 6]`` device tensor: entry ``[v, z]`` is the sum of the SSIM map over the
(h - 6)(w - 6) valid windows whose origin lies in z-layer ``z``.  ``afcm_amd.evaluation.evaluate_3D_from_stats`` adds the layers and divides by the
window count; the axial table of ``plane_metrics.plane_stats`` supplies the volume's PSNR and MAE.  Both inputs are read as they lie (any strides,
float32 / float16 / bfloat16, independently), the arithmetic is float64, every window a direct sum and free of atomics, so two calls on the same
inputs return the same bits.
"""
import torch

from ... import _lib
from .plane_metrics import C1, C2, WIN

TILE_Y, TILE_X = 16, 64                                   # window origins per workgroup: VS_TILE_Y x VS_TILE_X of csrc/metrics.hip


def volume_ssim_layers(ref, test, unit_map=False):
    """``[volumes, d, h, w]`` views ``ref`` / ``test`` (device tensors of one shape, every extent >= 7) -> float64 ``[volumes, d - 6]`` device
    tensor.  ``unit_map`` as in ``plane_stats``.  Asynchronous on the current stream; capturable."""
    _lib.require_gpu(ref, test)
    if ref.dim() != 4 or ref.shape != test.shape:
        raise RuntimeError(f'volume_ssim_layers: expected two [volumes, d, h, w] tensors of one shape, got {tuple(ref.shape)} and {tuple(test.shape)}')
    if ref.device != test.device:
        raise RuntimeError(f'volume_ssim_layers: tensors on {ref.device} and {test.device}')
    lib = _lib.load()
    volumes, d, h, w = (int(v) for v in ref.shape)
    layers = torch.empty([volumes, max(0, d - (WIN - 1))], dtype=torch.float64, device=ref.device)
    workspace = torch.empty([max(1, int(lib.afcm_volume_ssim_workspace_bytes(volumes, d, h, w)))], dtype=torch.uint8, device=ref.device)
    rc = lib.afcm_volume_ssim(layers.data_ptr(), ref.data_ptr(), test.data_ptr(), _lib.dtype_code(ref), _lib.dtype_code(test), volumes, d, h, w,
                              *ref.stride(), *test.stride(), int(bool(unit_map)), C1, C2, workspace.data_ptr(), _lib.stream_ptr(ref))
    _lib.launched(rc, 'volume_ssim')
    return layers

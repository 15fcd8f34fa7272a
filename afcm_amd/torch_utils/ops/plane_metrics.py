"""plane_stats: the per-plane statistics table behind the validation metrics (C ABI ``afcm_plane_metrics``, include/afcm_hip.h).

One call turns two stacks of planes into a float64 ``[planes, 8]`` device tensor -- extrema of both images, the three per-pixel sums of
PSNR / MAE and the sum of the 7 x 7 SSIM map -- from which ``afcm_amd.evaluation.*_from_stats`` finish the reference's numbers on the host.
Both inputs are read as they lie (any strides, float32 / float16 / bfloat16, independently), the arithmetic is float64 and free of atomics,
so two calls on the same inputs return the same bits.
"""
import torch

from ... import _lib

COLUMNS = ('max_ref', 'min_ref', 'max_test', 'min_test', 'sum_sq', 'sum_sq_maxnorm', 'sum_abs', 'sum_ssim')
WIN = 7
# scikit-image's SSIM constants at the data range the reference's calls end up with (float images, data_range = 2): (K1 L)^2, (K2 L)^2
C1, C2 = (0.01 * 2.0) ** 2, (0.03 * 2.0) ** 2


def plane_stats(ref, test, unit_map=False):
    """``[planes, h, w]`` views ``ref`` / ``test`` (device tensors of one shape) -> float64 ``[planes, 8]`` device tensor, columns as in
    ``COLUMNS``.  ``unit_map`` maps both from the network's [-1, 1] to [0, 1] on load (train.py:93-96, bit-identical to
    ``evaluation.to_unit_range``).  Asynchronous on the current stream; capturable."""
    _lib.require_gpu(ref, test)
    if ref.dim() != 3 or ref.shape != test.shape:
        raise RuntimeError(f'plane_stats: expected two [planes, h, w] tensors of one shape, got {tuple(ref.shape)} and {tuple(test.shape)}')
    if ref.device != test.device:
        raise RuntimeError(f'plane_stats: tensors on {ref.device} and {test.device}')
    lib = _lib.load()
    planes, h, w = (int(v) for v in ref.shape)
    table = torch.empty([planes, 8], dtype=torch.float64, device=ref.device)
    workspace = torch.empty([max(1, int(lib.afcm_plane_metrics_workspace_bytes(planes, h, w)))], dtype=torch.uint8, device=ref.device)
    rc = lib.afcm_plane_metrics(table.data_ptr(), ref.data_ptr(), test.data_ptr(), _lib.dtype_code(ref), _lib.dtype_code(test), planes, h, w,
                                *ref.stride(), *test.stride(), int(bool(unit_map)), C1, C2, workspace.data_ptr(), _lib.stream_ptr(ref))
    _lib.launched(rc, 'plane_metrics')
    return table

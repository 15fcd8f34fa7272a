"""The validation loop of the reference's trainer (train.py:84-105): EMA generator forward per batch, PSNR / SSIM / MAE of each batch,
means over the batches that count.  The caller keeps the checkpoint as `best` when ``ssim`` improves (train.py:108-111).

``metrics='device'`` computes each batch's statistics table on the device (afcm_plane_metrics) and leaves it there: the loop performs one
device -> host copy, and with it one synchronise, after the last batch.  ``metrics='host'`` is the reference's way -- copy both images to
the host, ``to_unit_range``, ``evaluation.evaluate_2D`` -- and exists as the comparison arm.
"""
import numpy as np
import torch

from . import evaluation, evaluation_device


def _host_batch(fake, real):
    pred = evaluation.to_unit_range(evaluation_device.as_planes(fake).float().cpu().numpy())[:, None, None]
    target = evaluation.to_unit_range(evaluation_device.as_planes(real).float().cpu().numpy())[:, None, None]
    return evaluation.evaluate_2D(pred, target)


def validate(step, batches, metrics='device'):
    """``step`` needs ``set_input(real_A, real_B)``, ``test()``, ``fake_B`` and ``real_B`` (network range, [N, 1, H, W]); ``batches`` yields
    ``(real_A, real_B)``.  Returns {'psnr', 'ssim', 'mae', 'batches', 'batches_counted'}: means of the per-batch means over the batches whose
    targets are not all empty (nan when none counts)."""
    if metrics not in ('device', 'host'):
        raise ValueError(f"metrics must be 'device' or 'host', got {metrics!r}")
    results, tables, shapes = [], [], []
    for real_A, real_B in batches:
        step.set_input(real_A, real_B)
        step.test()
        if metrics == 'host':
            results.append(_host_batch(step.fake_B, step.real_B))
        else:
            tables.append(evaluation_device.batch_stats(step.fake_B, step.real_B, from_network_range=True))
            shapes.append(tuple(int(v) for v in step.real_B.shape[-2:]))
    if tables:
        host = torch.cat(tables).cpu().numpy()                 # the loop's one copy and synchronise
        row = 0
        for t, (h, w) in zip(tables, shapes):
            results.append(evaluation.evaluate_2D_from_stats(host[row:row + t.shape[0]], h, w))
            row += t.shape[0]
    counted = [r for r in results if r is not None]
    mean = lambda k: float(np.mean([r[k] for r in counted])) if counted else float('nan')
    return {'psnr': mean(0), 'ssim': mean(1), 'mae': mean(2), 'batches': len(results), 'batches_counted': len(counted)}

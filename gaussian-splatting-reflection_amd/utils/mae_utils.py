"""Mean angular error of normals on the HIP path (reference: utils/mae_utils.py, used by eval_mae.py): `angular_error_map` and
`compute_mae` with the reference's names, shapes and two of its quirks, both on the fused kernel gsr_normal_mae
(csrc/gsr_metrics.hip): one pass over the two normal images instead of a dozen elementwise torch kernels.

  * compute_mae rescales by what the data holds: a prediction whose maximum exceeds 1 is divided by 255, a ground truth by 65535
    (utils/mae_utils.py:57-60).  The two `max()` tests are the reference's and, as there, wait for the device.
  * compute_mae returns `angular_error.mean()` of a map that holds NaN at invalid pixels: NaN as soon as one pixel is invalid.
"""
import torch

from _gsr import f32c
from gsr_eval import MetricsTable


def angular_error_map(pred, gt, eps=1e-8):
    """pred, gt: [3, H, W] float32 on the device.  Returns [H, W]: the angle between them in degrees, NaN where a norm is <= eps or the
    angle is NaN (utils/mae_utils.py:3-29)."""
    f32c(pred, "pred"), f32c(gt, "gt")       # the dtype errors of normals(), in front of the allocations below
    out = torch.empty(pred.shape[1:], dtype=torch.float32, device=pred.device)
    MetricsTable(1, pred.device).normals(0, pred, gt, eps=eps, error_map=out)
    return out


def compute_mae(pred, gt, eps=1e-8):
    """pred, gt: [1, 3, H, W]; pred in [0, 255] or [0, 1], gt in [0, 65535] or [0, 1].  Returns the mean angular error in degrees as a
    0-dim float32 tensor (utils/mae_utils.py:32-64)."""
    if pred.ndim != 4 or gt.ndim != 4:
        raise ValueError(f"Expected 4D tensors [B,3,H,W], got pred {pred.shape}, gt {gt.shape}")
    if pred.shape[0] != 1 or gt.shape[0] != 1:
        raise ValueError("This function expects batch size = 1")
    if pred.shape[1] != 3 or gt.shape[1] != 3:
        raise ValueError("Expected channel dimension = 3")
    pred, gt = pred[0].to(torch.float32), gt[0].to(torch.float32)
    pred_divisor = 255.0 if pred.max() > 1.0 else 1.0
    gt_divisor = 65535.0 if gt.max() > 1.0 else 1.0
    table = MetricsTable(1, pred.device)
    table.normals(0, pred, gt, pred_divisor=pred_divisor, gt_divisor=gt_divisor, eps=eps)
    angle_sum, valid, invalid = table.rows[0, 0], table.rows[0, 1], table.rows[0, 2]
    mean = torch.where(invalid > 0, torch.full_like(angle_sum, float("nan")), angle_sum / valid)
    return mean.to(torch.float32)

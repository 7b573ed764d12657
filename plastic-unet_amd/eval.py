"""Forward-only validation - drop-in for yaricom/Plastic-UNet src/eval.py (eval_net, :66-103).

The reference evaluates one sample at a time with a ZERO trace whose update is discarded (S5), a
BCE loss and fast_iou_metric on the host.  Here the samples go through the HIP forward in chunks
of ``batch`` slots (each slot with a zero trace - identical per-sample math), and the per-sample
loss / metric averages are the reference's.  By default the loss and the pixel counts the metrics
are made of come from one kernel call per chunk (kernels.seg_metrics) and one small table crosses
to the host per pass; metrics="host" keeps the numpy path, which gives the same bits.  tta="hflip"
(--tta hflip) scores the flip-averaged predictor of punet.augment.tta_forward instead, on either path.
"""
from optparse import OptionParser

import numpy as np
import torch

from punet import bce_loss
from punet import kernels as K
from punet import metrics as pm
from punet.augment import check_tta, tta_forward
from punet.fit import parse_fit
from utils import fast_iou_metric, iou_metric_batch, iou_score_from_counts


def _device_of(net):
    return next(net.parameters()).device


def _check_metrics(metrics):
    if metrics not in ("device", "host"):
        raise ValueError("metrics must be 'device' or 'host', not %r" % (metrics,))


def _forward_chunk(net, X, y, s, e, device, tta=None, fit=None):
    """Zero-trace forward of samples [s, e): (probabilities [B, n], targets [B, n]) on the device, both at the
    data size (fit: the FitSpec of a net of another side, punet/fit.py)."""
    xb = torch.from_numpy(np.asarray(X[s:e], dtype=np.float32)).to(device)
    tb = torch.from_numpy(np.asarray(y[s:e], dtype=np.float32)).to(device)
    B = xb.shape[0]
    out = tta_forward(net, xb, tta, fit)              # zero trace per slot; the update is discarded
    return out.reshape(B, -1), tb.reshape(B, -1)


def eval_net(net, X_val, y_val, device, criterion=None, debug=False, batch=32, metrics="device", tta=None, fit=None):
    """Returns (accuracy, loss) averaged over samples, as eval.py:66-103.

    metrics="device" (default, with criterion None): one kernels.seg_metrics call per chunk gives the
    per-sample loss (the bits of bce_loss on the sample) and the count of pixels on which target and
    thresholded prediction agree - fast_iou_metric on flattened vectors is exactly that count over
    the pixels -; one table comes back at the end and the host adds in sample order as before, so
    the two floats are the host path's, bit for bit.  With torch.distributed initialised on more
    than one rank (every rank calls this with the same data, as train.train does) the chunks are
    dealt round-robin to the ranks and merged by one all-reduce: every rank returns the same two
    numbers, the single process's.  metrics="host", or any criterion: the loss per slot and
    fast_iou_metric in numpy, every rank over the whole set.  fit: None, or the FitSpec of a net whose side is
    not the data's; the predictions come back to the data size on the device, where the loss and the counts
    are taken."""
    _check_metrics(metrics)
    check_tta(tta)
    net.eval()
    n = len(X_val)
    total_acc, total_loss = 0.0, 0.0
    if criterion is None and metrics == "device":
        world, rank = pm.world_and_rank()
        table = pm.MetricTable(n, 0, device)
        with torch.no_grad():
            for s, e in pm.chunks_for_rank(n, batch, world, rank):
                yf, tf = _forward_chunk(net, X_val, y_val, s, e, device, tta, fit)
                table.add(s, *K.seg_metrics(yf, tf))
        table.finish()
        pixels = int(np.asarray(y_val[0]).size) if n else 1
        for sample_loss in table.losses().tolist():
            total_loss += sample_loss
        for agree in table.agree().tolist():
            total_acc += agree / pixels
        return total_acc / n, total_loss / n
    with torch.no_grad():
        for s in range(0, n, batch):
            yf, tf = _forward_chunk(net, X_val, y_val, s, s + batch, device, tta, fit)
            B = yf.shape[0]
            losses = torch.stack([criterion(yf[b], tf[b]) if criterion is not None else bce_loss(yf[b], tf[b])
                                  for b in range(B)])
            # one device->host copy per chunk; the per-sample sums in the reference's order
            for sample_loss in losses.cpu().tolist():
                total_loss += sample_loss
            y_np, t_np = yf.cpu().numpy(), tf.cpu().numpy()
            for b in range(B):
                total_acc += fast_iou_metric(y_true_in=t_np[b], y_pred_in=y_np[b])
    return total_acc / n, total_loss / n


def iou_sweep(net, X, y, device, thresholds, batch=32, metrics="device", tta=None, fit=None):
    """The competition IoU score (iou_metric_batch) of the zero-trace predictions at every threshold:
    a float32 array, one score per threshold.

    metrics="device" (default): the targets go up per chunk next to the images, kernels.seg_metrics
    counts per sample and threshold the predicted pixels and those that are foreground targets too,
    and nothing but the count table comes back; utils.iou_score_from_counts - the tail of
    iou_metric_batch - turns the counts into the scores.  The thresholds must be strictly ascending
    (32 per kernel call; a longer list takes more calls).  metrics="host": every prediction comes
    back and iou_metric_batch runs per threshold in numpy.  The same bits either way.  Always the
    whole set on the calling process, whatever the process group.  fit: as in eval_net - the counts are
    taken at the data size."""
    _check_metrics(metrics)
    check_tta(tta)
    net.eval()
    thresholds = [float(th) for th in thresholds]
    if metrics == "host":
        preds = []
        with torch.no_grad():
            for s in range(0, len(X), batch):
                xb = torch.from_numpy(np.asarray(X[s:s + batch], dtype=np.float32)).to(device)
                out = tta_forward(net, xb, tta, fit)
                preds.append(out.cpu().numpy().reshape(xb.shape[0], 1, 1, out.shape[-2], out.shape[-1]))
        preds = np.concatenate(preds, 0)
        return np.array([iou_metric_batch(y, preds > np.float64(th)) for th in thresholds])
    n = len(X)
    groups = [thresholds[k:k + 32] for k in range(0, len(thresholds), 32)]
    tables = [pm.MetricTable(n, len(g), device) for g in groups]
    with torch.no_grad():
        for s, e in pm.chunks_for_rank(n, batch):
            yf, tf = _forward_chunk(net, X, y, s, e, device, tta, fit)
            for g, table in zip(groups, tables):
                table.add(s, *K.seg_metrics(yf, tf, g))
    scores = []
    for g, table in zip(groups, tables):
        table.finish(across_ranks=False)
        scores += [iou_score_from_counts(table.icount(k), table.tcount(), table.pcount(k)) for k in range(len(g))]
    return np.array(scores)


def score_model_best_iou(net, X_valid, y_valid, device, debug=False, batch=32, metrics="device", tta=None, fit=None):
    """Threshold search by the best competition IoU (eval.py:20-64): zero-trace forward of every
    validation sample, 31 thresholds linspace(0.3, 0.7) mapped through the logit as the reference
    does, the score of iou_sweep per threshold; returns (threshold_best, iou_best).

    The reference compares its Python LIST of predictions with a float (eval.py:52), which raises
    TypeError on Python 3; here the predictions are compared as one array
    [N, 1, 1, H, W] - the comparison the reference intends - so the search completes."""
    thresholds_ori = np.linspace(0.3, 0.7, 31)
    thresholds = np.log(thresholds_ori / (1 - thresholds_ori))
    ious = iou_sweep(net, X_valid, y_valid, device, thresholds, batch=batch, metrics=metrics, tta=tta, fit=fit)
    if debug:
        print(ious)
    k = int(np.argmax(ious))
    return thresholds[k], ious[k]


def get_args():
    parser = OptionParser()
    parser.add_option('--model', '-m', default='MODEL.pth', help="the file with the model state_dict")
    parser.add_option('-i', '--data', dest='data_dir', type='string', help='dataset .npz (x_valid, y_valid)')
    parser.add_option('-g', '--gpu', action='store_true', dest='gpu', default=True, help='use the GPU (always)')
    parser.add_option('-v', '--debug', action='store_true', dest='debug', default=False)
    parser.add_option('--model-type', dest='model_type', default='unetpres', help='unetpres | unetp')
    parser.add_option('--nbf', dest='nbf', type='int', default=101, help="the net's side")
    parser.add_option('--tta', dest='tta', default=None, type='choice', choices=['hflip'],
                      help="test-time augmentation: hflip scores the mean of each prediction and its mirror's")
    parser.add_option('--fit', dest='fit', default=None, type='choice', choices=['pad', 'resize'],
                      help="the data's size (from the file) differs from --nbf: reflect-pad or resize each batch to the "
                           "net's side on the device and bring every prediction back before it is scored")
    (options, args) = parser.parse_args()
    return options


if __name__ == "__main__":
    args = get_args()
    device = torch.device('cuda')
    from unet import UNetp, UNetpRes
    cls = UNetpRes if args.model_type == 'unetpres' else UNetp
    net = cls(n_channels=1, n_classes=1, device=device, nbf=args.nbf)
    net.load_state_dict(torch.load(args.model, weights_only=True))
    d = np.load(args.data_dir)
    fit = parse_fit(args.fit, d["x_valid"].shape[-2:], args.nbf)
    acc, loss = eval_net(net, d["x_valid"], d["y_valid"], device, tta=args.tta, fit=fit)
    print("Validation accuracy: %f, loss: %f" % (acc, loss))

"""Mask inference - drop-in for yaricom/Plastic-UNet src/infer.py: inference (:28-48), predict
(:50-108), start_inference (:110-179) and the CLI (:181-263).

Forward-only with a zero trace per image (S5); the HIP forward runs in chunks of ``batch`` images
(each slot with its own zero trace: the per-image math of the reference).  predict() thresholds
the probabilities, RLE-encodes (column-major, utils/rle_encode.py) and writes the submission CSV
with the reference's columns (id, rle_mask).  The threshold and the encoding run on the device
(predict_rle, kernels.rle_encode: only the runs come to the host); rle="host" is the reference's
host code on the probability maps.  start_inference() builds the reference's model
(UNetpRes at the image width), loads the state dict with the weights-only loader, picks the mask
threshold with eval.score_model_best_iou (whose reference version raises at S12 - see there) and
predicts.  ``tta="hflip"`` (--tta hflip) on any of them: every prediction is the mean of the net's output
on the image and its un-mirrored output on the mirrored image, merged on the device
(punet.augment.tta_forward), so the threshold search, the threshold and the encoding see that predictor.
``fit=`` (--fit pad|resize --net-size S): the net's side S is not the images'; every batch is fitted to S on the
device and every prediction brought back (punet/fit.py), so all of the above stays at the images' size.
"""
import csv
import os
from optparse import OptionParser

import numpy as np
import torch

from punet import kernels as K
from punet.augment import check_tta, tta_forward
from punet.fit import parse_fit
from punet.rle import RunTable, compare_value
from utils import encode


def inference(net, img_data, device):
    """One image [C,H,W] -> probability mask [H,W] (numpy), as infer.py:28-48."""
    return predict_masks(net, np.asarray(img_data)[None], device)[0]


def predict_masks(net, X, device, batch=32, tta=None, fit=None):
    """Probability masks [N,H,W] of images X [N,C,H,W], zero trace per image.  fit: None, or the FitSpec
    (punet/fit.py) of a net whose side is not H: the masks come back at the images' size all the same."""
    check_tta(tta)
    net.eval()
    out = []
    with torch.no_grad():
        for s in range(0, len(X), batch):
            xb = torch.from_numpy(np.asarray(X[s:s + batch], dtype=np.float32)).to(device)
            y = tta_forward(net, xb, tta, fit)
            out.append(y.cpu().numpy())
    return np.concatenate(out, 0)


def _check_rle(rle):
    if rle not in ("device", "host"):
        raise ValueError("rle must be 'device' or 'host', not %r" % (rle,))


def predict_rle(net, X, device, thr, batch=32, keep=None, tta=None, fit=None):
    """The strings encode(np.round(m > thr)) of the probability masks m of images X [N,C,H,W], with
    the threshold and the encoding on the device: per chunk only the run table comes back.  Chunk
    i + 1's forward and encode are enqueued before chunk i's table is read, so the device works while
    the host prints; the buffers of at most two chunks are alive.  ``keep``: a list that receives each
    chunk's probability maps on the host (for the PNG masks).  fit: as in predict_masks - the runs are those
    of the masks at the images' size."""
    check_tta(tta)
    net.eval()
    th = compare_value(thr)
    out, waiting = [], None
    with torch.no_grad():
        for s in range(0, len(X), batch):
            xb = torch.from_numpy(np.asarray(X[s:s + batch], dtype=np.float32)).to(device)
            y = tta_forward(net, xb, tta, fit)
            table = RunTable(*K.rle_encode(y.contiguous(), th))
            if waiting is not None:
                out.extend(waiting.strings())
            waiting = table
            if keep is not None:
                keep.append(y.cpu().numpy())
    if waiting is not None:
        out.extend(waiting.strings())
    return out


def _write_mask_png(path, mask):
    from PIL import Image
    tmp = (np.squeeze(mask).astype(np.uint8) * 255)
    Image.fromarray(np.dstack((tmp, tmp, tmp))).save(path)


def predict(net, test_df, params, visualize=False, save_masks=False, rle="device", tta=None, fit=None):
    """Threshold + RLE + CSV (infer.py:50-108).  test_df: the reference's test frame (index = image
    ids, column ``images``), or a pair (ids, X_test [N,C,H,W]).  params: out_dir, mask_threshold,
    img_chan/img_height/img_width (to shape the images), subm_file, device (default: the net's).
    ``visualize`` (matplotlib windows in the reference) is not supported on this host-less path.
    rle: "device" (default) thresholds and encodes on the device, and the probability maps come back
    only for ``save_masks``; "host" brings every map back and encodes it with utils.encode.  Both give
    the same rows.  tta: None or "hflip" (default: params.get("tta")), on either path.  fit: None or a FitSpec
    (default: params.get("fit")): the net's side differs from the images'; masks, PNGs and rows stay at the
    images' size."""
    _check_rle(rle)
    tta = params.get("tta") if tta is None else tta
    check_tta(tta)
    fit = params.get("fit") if fit is None else fit
    if isinstance(test_df, tuple):
        ids, X_test = test_df
        ids = list(ids)
    else:
        ids = list(test_df.index)
        X_test = np.array(test_df.images.tolist()).reshape(-1, params["img_chan"], params["img_height"],
                                                             params["img_width"])
    print("Start prediction with the number of test image samples:", len(ids))
    device = params.get("device") or next(net.parameters()).device
    thr = params["mask_threshold"]
    if rle == "device":
        kept = [] if save_masks else None
        codes = predict_rle(net, X_test, device, thr, keep=kept, tta=tta, fit=fit)
        masks = np.concatenate(kept, 0) if kept else ()
    else:
        masks = predict_masks(net, X_test, device, tta=tta, fit=fit)
    if save_masks:
        os.makedirs(os.path.join(params["out_dir"], "masks"), exist_ok=True)
        for fn, m in zip(ids, masks):
            _write_mask_png(os.path.join(params["out_dir"], "masks", "%s.png" % fn), m > thr)
    if rle == "device":
        rows = list(zip(ids, codes))
    else:
        rows = [(fn, encode(np.round(m > thr))) for fn, m in zip(ids, masks)]
    path = os.path.join(params["out_dir"], params.get("subm_file", "submission.csv"))
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["id", "rle_mask"])
        w.writerows(rows)
    print("Results encoded to:", path)
    return rows


def start_inference(model, test_df, X_valid, y_valid, out_dir, img_width, img_height, img_chan,
                    subm_file="submission.csv", gpu=True, visualize=False, save_masks=False, debug=False,
                    mask_threshold=None, model_type="unetpres", rle="device", tta=None, fit=None):
    """infer.py:110-179: the reference builds UNetpRes(n_channels=img_chan, n_classes=1,
    nbf=img_width), loads ``model`` (a state_dict path), scores the best threshold on the
    validation set and predicts.  ``mask_threshold`` skips the threshold search; ``model_type``
    'unetp' loads a UNetp instead.  The product path is the GPU one (``gpu`` is accepted for the
    signature; there is no CPU fallback).  ``rle``: as in predict.  ``tta`` goes to the threshold search and
    to the prediction alike: the threshold is chosen for the predictor that is submitted.  ``fit``: None, or the
    FitSpec of data img_height x img_width on a net of side fit.side: the net is built at that side, the
    threshold search scores and the submission encodes the predictions brought back to the data size."""
    _check_rle(rle)
    check_tta(tta)
    fit = parse_fit(fit)
    if fit and (fit.h, fit.w) != (img_height, img_width):
        raise ValueError("fit: a spec for %d x %d data, images of %d x %d" % (fit.h, fit.w, img_height, img_width))
    from unet import UNetp, UNetpRes
    import eval as ev
    device = torch.device("cuda")
    cls = UNetpRes if model_type == "unetpres" else UNetp
    net = cls(n_channels=img_chan, n_classes=1, nbf=fit.side if fit else img_width, device=device)
    print("Loading model %s" % (model,))
    sd = model if isinstance(model, dict) else torch.load(model, map_location="cpu", weights_only=True)
    net.load_state_dict(sd)
    net.to(device)
    if mask_threshold is None:
        print("Score model for best IoU")
        mask_threshold, iou_best = ev.score_model_best_iou(net, X_valid, y_valid, device, debug=debug, tta=tta, fit=fit)
        print("Best threshold: %f, best IoU: %f" % (mask_threshold, iou_best))
    os.makedirs(out_dir, exist_ok=True)
    params = {"out_dir": out_dir, "device": device, "img_width": img_width, "img_height": img_height,
              "img_chan": img_chan, "mask_threshold": mask_threshold, "subm_file": subm_file, "debug": debug}
    return predict(net, test_df, params, visualize=visualize, save_masks=save_masks, rle=rle, tta=tta, fit=fit)


def get_args():
    parser = OptionParser()
    parser.add_option('--model', '-m', default='MODEL.pth',
                      help="Specify the file in which is stored the model (default : 'MODEL.pth')")
    parser.add_option('-i', '--data', dest='data_dir', type='string', help='the directory with input test data')
    parser.add_option('--out', '-o', dest='out_dir', default='./out', help='directory for ouput images')
    parser.add_option('-g', '--gpu', action='store_true', dest='gpu', default=True, help='use the GPU (always)')
    parser.add_option('--visualize', '-v', action='store_true', default=False)
    parser.add_option('--save', '-s', action='store_true', default=False, help="To save the output masks")
    parser.add_option('--mask-threshold', '-t', dest='mask_threshold', type=float,
                      help="Minimum probability value to consider a mask pixel white")
    parser.add_option('--partial', '-p', action='store_true', default=False)
    parser.add_option('--partial-size', '-d', dest='partial_size', default=100, type='int')
    parser.add_option('--model-type', dest='model_type', default='unetpres', help='unetpres | unetp')
    parser.add_option('--rle', dest='rle', default='device', type='choice', choices=['device', 'host'],
                      help="where the masks are thresholded and run-length encoded: device | host")
    parser.add_option('--tta', dest='tta', default=None, type='choice', choices=['hflip'],
                      help="test-time augmentation: hflip averages each prediction with that of the mirrored image")
    parser.add_option('--fit', dest='fit', default=None, type='choice', choices=['pad', 'resize'],
                      help="run the 101 x 101 images on a net of side --net-size: reflect-pad or resize each batch on the "
                           "device; the predictions come back to 101 x 101 before the threshold and the encoding")
    parser.add_option('--net-size', dest='net_size', type='int', default=None, help="the net's side with --fit")
    (options, args) = parser.parse_args()
    return options


if __name__ == "__main__":
    args = get_args()
    os.makedirs(args.out_dir, exist_ok=True)
    if args.data_dir is None:
        raise ValueError("The input data directory or dataset file not specified")
    from utils import load_test_dataset, load_train_dataset
    w = h = 101
    c = 1
    if (args.fit is None) != (args.net_size is None):
        raise ValueError("--fit and --net-size go together")
    fit = parse_fit(args.fit, (h, w), args.net_size)
    test_df = load_test_dataset(args.data_dir, w, h, c, partial=args.partial, part_size=args.partial_size)
    x_train, x_valid, y_train, y_valid = load_train_dataset(args.data_dir, w, h, c)
    if args.partial:
        x_valid = x_valid[:args.partial_size]
        y_valid = y_valid[:args.partial_size]
    start_inference(model=args.model, test_df=test_df, X_valid=x_valid, y_valid=y_valid, out_dir=args.out_dir,
                    gpu=args.gpu, img_width=w, img_height=h, img_chan=c, visualize=args.visualize,
                    save_masks=args.save, debug=True, mask_threshold=args.mask_threshold,
                    model_type=args.model_type, rle=args.rle, tta=args.tta, fit=fit)

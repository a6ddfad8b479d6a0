"""Mirror of DOTA_devkit/ResultMerge_multi_process.py, the merge the reference's evaluation tools run
(tools/parse_pkl/parse_pkl_mege_results_for_dota_evaluation.py): per-class Task1 result files of image PATCHES ->
coordinates mapped back to the original image -> `py_cpu_nms_poly_fast` per (class, image) at `nms_thresh = 0.1` ->
merged files.  Same function names, file formats, patch-name grammar (`<image>__<rate>__<x>___<y>`) and defaults;
`mergebypoly(srcpath, dstpath)` is the entry point (ResultMerge_multi_process.py:249-262).

The polygon NMS runs on the MI355X: all (image) segments of one class file go through ONE `orp_poly_nms_f64_batched`
launch sequence with the HBB pre-filter (`py_gpu_nms_poly_fast`).  The visiting order of every segment is numpy's
`scores.argsort()[::-1]`, taken on the host exactly as the reference takes it (ties included), and passed as presorted.
"""
import os
import re

import numpy as np
import torch

from ..mmdet_ops.nms_wrapper import poly_nms_f64_batched_device
from .result_merge import GetFileFromThisRootDir, custombasename, poly2origpoly, py_cpu_nms  # noqa: F401

# the thresh for nms when merge image (ResultMerge_multi_process.py:21)
nms_thresh = 0.1


def py_gpu_nms_poly_fast_segments(dets_list, thresh, device=None, hbb_prefilter=True):
    """[dets [n_s,9] float64 (8 coords + score)] -> [kept ORIGINAL indices of segment s in visiting order], each identical
    to `py_cpu_nms_poly_fast(dets_s, thresh)` (hbb_prefilter=False: `py_cpu_nms_poly`); one launch sequence for all."""
    dets_list = [np.asarray(d, dtype=np.float64).reshape(-1, 9) for d in dets_list]
    sizes = [d.shape[0] for d in dets_list]
    if sum(sizes) == 0:
        return [[] for _ in dets_list]
    orders = [d[:, 8].argsort()[::-1] for d in dets_list]
    cat = np.ascontiguousarray(np.concatenate([d[o] for d, o in zip(dets_list, orders)]))
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    keep, num = poly_nms_f64_batched_device(torch.from_numpy(cat).to(dev), torch.from_numpy(off).to(dev), max(sizes),
                                            thresh, hbb_prefilter=hbb_prefilter, presorted=True)
    keep, num = keep.cpu().numpy(), num.cpu().numpy()
    return [[int(i) for i in o[keep[s0:s0 + k] - s0]] for o, s0, k in zip(orders, off[:-1], num)]


def py_gpu_nms_poly_fast(dets, thresh, device=None):
    """dets [N,9] float64 -> kept ORIGINAL indices in visiting order, identical to `py_cpu_nms_poly_fast(dets, thresh)`
    (ResultMerge_multi_process.py:60-121: fp64 HBB overlap first, polyiou only where it is > 0)."""
    return py_gpu_nms_poly_fast_segments([dets], thresh, device)[0]


# nmsbynamedict hands all images of a file to this in one call
py_gpu_nms_poly_fast.segments = py_gpu_nms_poly_fast_segments


def nmsbynamedict(nameboxdict, nms, thresh):
    """ResultMerge_multi_process.py:156-172.  An `nms` with a `segments` attribute receives every image at once."""
    names = list(nameboxdict)
    segments = getattr(nms, 'segments', None)
    if segments is not None:
        keeps = segments([np.array(nameboxdict[n]) for n in names], thresh)
    else:
        keeps = [nms(np.array(nameboxdict[n]), thresh) for n in names]
    return {n: [nameboxdict[n][index] for index in keep] for n, keep in zip(names, keeps)}


_PAT_XY = re.compile(r'__\d+___\d+')
_PAT_RATE = re.compile(r'__([\d+\.]+)__\d+___')


def mergesingle(dstpath, nms, fullname):
    """ResultMerge_multi_process.py:182-223: one result file of srcpath -> a merged file of the same name in dstpath."""
    name = custombasename(fullname)
    dstname = os.path.join(dstpath, name + '.txt')
    with open(fullname, 'r') as f_in:
        nameboxdict = {}
        for splitline in [x.strip().split(' ') for x in f_in.readlines()]:
            subname = splitline[0]
            oriname = subname.split('__')[0]
            x_y = re.findall(_PAT_XY, subname)
            x_y_2 = re.findall(r'\d+', x_y[0])
            x, y = int(x_y_2[0]), int(x_y_2[1])
            rate = re.findall(_PAT_RATE, subname)[0]
            confidence = splitline[1]
            poly = list(map(float, splitline[2:]))
            det = poly2origpoly(poly, x, y, rate)
            det.append(confidence)
            det = list(map(float, det))
            nameboxdict.setdefault(oriname, []).append(det)
        nameboxnmsdict = nmsbynamedict(nameboxdict, nms, nms_thresh)
        with open(dstname, 'w') as f_out:
            for imgname in nameboxnmsdict:
                for det in nameboxnmsdict[imgname]:
                    f_out.write(imgname + ' ' + str(det[-1]) + ' ' + ' '.join(map(str, det[0:-1])) + '\n')


def mergebase(srcpath, dstpath, nms):
    """ResultMerge_multi_process.py:233-236: the files one after the other."""
    for filename in GetFileFromThisRootDir(srcpath):
        mergesingle(dstpath, nms, filename)


def mergebase_parallel(srcpath, dstpath, nms):
    """ResultMerge_multi_process.py:225-231 spreads the files over a 16-process CPU pool.  Here every file is one
    device launch sequence on the current GPU, so the files run one after the other in this process; the output is
    the same."""
    mergebase(srcpath, dstpath, nms)


def mergebyrec(srcpath, dstpath):
    mergebase(srcpath, dstpath, py_cpu_nms)


def mergebypoly(srcpath, dstpath):
    """srcpath: result files before merge and nms; dstpath: result files after merge and nms
    (ResultMerge_multi_process.py:249-262), with the fast polygon NMS on the GPU."""
    mergebase_parallel(srcpath, dstpath, py_gpu_nms_poly_fast)

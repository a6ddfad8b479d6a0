"""Why the benchmark's detections differ with ORP_BN_DOWNSAMPLE_CONV_FUSE on: stage by stage, then row by row.
Two models built exactly as bench.py builds them (seed 0, image seed 1234, calibrate_head under the side's own switch).

    [DET=0] [OUT=DIR] python tests/checks/explain_dump_rows.py

DET=0: the library's deterministic mode off, as bench.py leaves it while its own step is reproducible (default: on, so that switch off
against switch off again is a noise floor of exactly 0).  OUT=DIR: the final rows of both sides as DIR/explain_rows_{off,on}.npz."""
import os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import bench
from orientedreppoints_amd import switches
from orientedreppoints_amd.mmdet_models import ConfigDict, build_detector
from orientedreppoints_amd.mmdet_models import orientedreppoints_head as head_mod
from oracle import orp_oracle as O

dev = torch.device('cuda:0')
torch.backends.cudnn.deterministic = os.environ.get('DET', '1') == '1'      # (bench.py leaves it off while its step is reproducible)
THR = float(bench.TEST_CFG['score_thr'])
IOU = 0.4
P = lambda *a: print(*a, flush=True)


def build(flag):
    switches.BN_DOWNSAMPLE_CONV_FUSE = flag
    torch.manual_seed(0)
    model = build_detector(ConfigDict(bench.MODELS['r50']), train_cfg=None, test_cfg=ConfigDict(bench.TEST_CFG)).to(dev).eval()
    g = torch.Generator(device='cpu').manual_seed(1234)
    img = torch.randn(1, 3, 1024, 1024, generator=g).to(dev)
    bench.calibrate_head(model, img[:1])
    return model, img


def run(model, img, flag):
    switches.BN_DOWNSAMPLE_CONV_FUSE = flag
    out = {}
    blocks = {}
    hooks = []
    for name, m in model.backbone.named_modules():
        if type(m).__name__ == 'Bottleneck':
            hooks.append(m.register_forward_hook(lambda mod, i, o, name=name: blocks.__setitem__(name, o.detach().clone())))
    cap = {}
    orig = head_mod.multiclass_rnms

    def spy(multi_bboxes, multi_scores, score_thr, *a, **k):
        cap['boxes'] = multi_bboxes.detach().clone(); cap['scores'] = multi_scores.detach().clone()
        return orig(multi_bboxes, multi_scores, score_thr, *a, **k)
    head_mod.multiclass_rnms = spy
    static = model.test_cfg.get('static_postprocess', True)
    metas = [dict(img_shape=(1024, 1024, 3), pad_shape=(1024, 1024, 3), scale_factor=1.0, flip=False)]
    try:
        with torch.no_grad():
            c = model.backbone(img)
            for h in hooks:
                h.remove()
            p = model.neck(c)
            head_out = model.bbox_head(p)
            out['static'] = model.simple_test_batch(img, metas)[0]
            model.test_cfg['static_postprocess'] = False
            out['final'] = model.simple_test(img, metas)
    finally:
        head_mod.multiclass_rnms = orig
        model.test_cfg['static_postprocess'] = static
    out['head'] = [[t.clone().float() for t in lvl] if isinstance(lvl, (list, tuple)) else lvl for lvl in head_out]
    out.update(blocks=blocks, c=[t.clone() for t in c], p=[t.clone().float() for t in p], cap=cap)
    return out


def rel(a, b):
    return float((a.float() - b.float()).abs().max()) / max(float(b.float().abs().max()), 1e-30)


m_off, img = build(False)
m_on, _ = build(True)
P('cls_out.bias calibrated under on vs under off: max |diff| %.3g' % float((m_on.bbox_head.reppoints_cls_out.bias - m_off.bbox_head.reppoints_cls_out.bias).abs().max()))
off, off2, on = run(m_off, img, False), run(m_off, img, False), run(m_on, img, True)

P('\n== stage by stage: max |a - b| / max |b|;  on vs off  |  off vs off again (the noise floor)')
for k in off['blocks']:
    P('backbone %-10s %.3g | %.3g' % (k, rel(on['blocks'][k], off['blocks'][k]), rel(off2['blocks'][k], off['blocks'][k])))
for i in range(len(off['p'])):
    P('FPN level %d         %.3g | %.3g' % (i, rel(on['p'][i], off['p'][i]), rel(off2['p'][i], off['p'][i])))
for j, grp in enumerate(off['head']):
    if isinstance(grp, (list, tuple)):
        for i, t in enumerate(grp):
            if torch.is_tensor(t):
                P('head output %d level %d: max |on - off| %.3g at max |off| %.3g | off again %.3g' % (j, i, float((on['head'][j][i] - t).abs().max()), float(t.abs().max()), float((off2['head'][j][i] - t).abs().max())))

P('\n== candidates handed to the NMS (every point of the nms_pre top-k per level, 15 class scores each)')
bo, so, bn_, sn = off['cap']['boxes'], off['cap']['scores'][:, 1:], on['cap']['boxes'], on['cap']['scores'][:, 1:]
P('points: off %d, on %d; (point, class) pairs above %.2f: off %d, on %d' % (bo.size(0), bn_.size(0), THR, int((so > THR).sum()), int((sn > THR).sum())))
# match the points of the two sides by their boxes
d = torch.cdist(bn_[:, -8:].double(), bo[:, -8:].double(), p=float('inf'))
near, idx = d.min(1)
P('points of "on" with a point of "off" within 0.05 px: %d of %d (largest distance among them %.3g px); without: %d (the nms_pre top-k boundary)' % (int((near < 0.05).sum()), bn_.size(0), float(near[near < 0.05].max()), int((near >= 0.05).sum())))
def max_coordinate(boxes, scores):
    return float(boxes[(scores > THR).any(1)][:, -8:].max())


max_off, max_on = max_coordinate(bo, so), max_coordinate(bn_, sn)
P('largest candidate coordinate (the class offset of the NMS is label x (this + 1), added in fp32): off %.6f, on %.6f' % (max_off, max_on))


def nms_keep(boxes, scores, mx):
    """multiclass_rnms' own steps on these candidates with the class offset label x (mx + 1): the kept (point, class) pairs"""
    from orientedreppoints_amd.mmdet_ops import rnms
    valid = scores > THR
    b = boxes[:, None, -8:].expand(-1, scores.size(1), 8)[valid]
    labels = valid.nonzero()[:, 1]
    offs = labels.to(b) * (torch.tensor(float(mx), dtype=torch.float32, device=dev) + 1)
    _dets, keep = rnms(torch.cat([b + offs[:, None], scores[valid][:, None]], 1), IOU)
    pairs = valid.nonzero()[keep.long()]
    return {(int(p), int(l)) for p, l in pairs.tolist()}


P('\n== the class offset alone: the SAME candidates of the off side through the NMS, the largest coordinate moved by one fp32 ulp at a time')
m0 = np.float32(max_off)
base = nms_keep(bo, so, m0)
P('offset from %.7f (as the model runs it): %d rows kept' % (float(m0), len(base)))
m = m0
for step in range(1, 4):
    m = np.nextafter(m, np.float32(0))
    k = nms_keep(bo, so, m)
    P('offset from %.7f (%d ulp lower, %.3g px): %d rows kept, %d only here, %d only at the model\'s offset; their classes %s'
      % (float(m), step, float(m0) - float(m), len(k), len(k - base), len(base - k), sorted(l for _p, l in (k ^ base))))
P('\n== final detections row by row (per class: rows [k, 27] = 9 points, 4 corners, score)')
same_static = all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(off['static'], off['final']))
P('the captured-path rows (what --dump-outputs writes) equal the reference-shaped path rows on the off side: %s' % same_static)
tot = dict(matched=0, thr=0, nms=0, topk=0, cascade=0, rect=0, other=0)
worst_c, worst_s, worst_r, rect_flips = 0.0, 0.0, 0.0, []
for c, (a, b) in enumerate(zip(off['final'], on['final'])):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    dist = np.abs(a[:, None, :18] - b[None, :, :18]).max(-1) if len(a) and len(b) else np.zeros((len(a), len(b)))
    ma = dist.min(1) < 0.05 if len(b) else np.zeros(len(a), bool)
    mb = dist.min(0) < 0.05 if len(a) else np.zeros(len(b), bool)
    j = dist.argmin(1)
    if ma.any():
        cd = np.abs(a[ma][:, 18:26] - b[j[ma]][:, 18:26]).max(1)
        for q in np.nonzero(cd >= 0.05)[0]:
            rect_flips.append((c, float(a[ma][q, 26]), float(cd[q]), float(np.abs(a[ma][q, :18] - b[j[ma]][q, :18]).max())))
        worst_r = max(worst_r, float(cd[cd < 0.05].max()) if (cd < 0.05).any() else 0.0)
        worst_c = max(worst_c, float(np.abs(a[ma][:, :18] - b[j[ma]][:, :18]).max())); worst_s = max(worst_s, float(np.abs(a[ma][:, 26] - b[j[ma]][:, 26]).max()))
    order_same = bool(ma.all() and mb.all() and len(a) == len(b) and np.array_equal(j, np.arange(len(a))))
    P('class %2d: off %3d rows, on %3d rows, matched %3d, same order %s' % (c, len(a), len(b), int(ma.sum()), order_same))
    tot['matched'] += int(ma.sum())
    for side, rows, other, mask, omask, cand_b, cand_s in (('off', a, b, ma, mb, bn_, sn), ('on', b, a, mb, ma, bo, so)):
        for r in rows[~mask]:
            # the same point among the OTHER side's candidates, its score for this class there
            dd = (cand_b[:, -8:].double() - torch.from_numpy(r[18:26]).to(dev)).abs().max(1).values
            k = int(dd.argmin())
            if float(dd[k]) >= 0.05:
                tot['topk'] += 1
                P('   only in %-3s: score %.6f -- its point is not among the other side\'s candidates (nearest %.3g px): nms_pre top-k boundary' % (side, r[26], float(dd[k])))
                continue
            s_other = float(cand_s[k, c])
            if s_other <= THR:
                tot['thr'] += 1
                P('   only in %-3s: score %.6f, on the other side %.6f <= %.2f: the score threshold, |score - thr| %.2g and %.2g' % (side, r[26], s_other, THR, abs(r[26] - THR), abs(s_other - THR)))
                continue
            # a candidate on both sides with the same box, kept on this side only: the other side's NMS suppressed it.  The NMS sees
            # fp32 coordinates + label * (largest candidate coordinate + 1) (multiclass_rnms' class offset), so the IoUs are taken on
            # those, each side with its own offset
            mx_x, mx_y = (max_off, max_on) if side == 'off' else (max_on, max_off)
            ofs = lambda v, mx: (np.asarray(v, dtype=np.float32) + np.float32(c) * (np.float32(mx) + np.float32(1))).astype(np.float32)
            r_y = cand_b[k, -8:].float().cpu().numpy()
            hi = other[other[:, 26] > s_other - 2e-7]
            iou_y = O.quad_iou_matrix(np.ascontiguousarray(ofs(r_y[None], mx_y)), np.ascontiguousarray(ofs(hi[:, 18:26], mx_y)))[0] if len(hi) else np.zeros(0)
            if not len(hi) or iou_y.max() <= IOU:
                tot['other'] += 1
                P('   only in %-3s: class %d score %.6f (other side %.6f): no kept row of the other side overlaps it by more than %.1f on the offset coordinates (largest IoU %.4f)   <-- unexplained' % (side, c, r[26], s_other, IOU, float(iou_y.max()) if len(hi) else 0.0))
                continue
            K = hi[int(iou_y.argmax())]
            dk = np.abs(rows[:, :18] - K[None, :18]).max(1)
            if dk.min() >= 0.05:
                tot['cascade'] += 1
                P('   only in %-3s: class %d score %.6f: suppressed on the other side (IoU %.4f) by the row of score %.6f, which only the other side has: follows from that row' % (side, c, r[26], float(iou_y.max()), K[26]))
                continue
            Kx = rows[int(dk.argmin())]
            cdk = float(np.abs(Kx[18:26] - K[18:26]).max())
            iou_x = float(O.quad_iou_matrix(np.ascontiguousarray(ofs(r[None, 18:26], mx_x)), np.ascontiguousarray(ofs(Kx[None, 18:26], mx_x)))[0, 0])
            iou_plain = float(O.quad_iou_matrix(np.ascontiguousarray(r[None, 18:26], dtype=np.float32), np.ascontiguousarray(Kx[None, 18:26], dtype=np.float32))[0, 0])
            if cdk >= 0.05:
                tot['rect'] += 1
                P('   only in %-3s: class %d score %.6f: suppressed on the other side (IoU %.4f) by the row of score %.6f, whose min-area-rect is another rectangle there (corners %.3g px apart, a tie listed below); with this side\'s rectangle the IoU is %.4f' % (side, c, r[26], float(iou_y.max()), K[26], cdk, iou_x))
            elif iou_x <= IOU:
                tot['nms'] += 1
                P('   only in %-3s: class %d score %.6f against the row of score %.6f: IoU %.4f <= %.1f on this side\'s offset coordinates (offset %d x (%.4f + 1)), %.4f > %.1f on the other side\'s (%d x (%.4f + 1)); without the offset %.4f.  The class offset moved by %.3g and rounds the corners elsewhere'
                  % (side, c, r[26], K[26], iou_x, IOU, c, mx_x, float(iou_y.max()), IOU, c, mx_y, iou_plain, abs(c * (mx_x - mx_y))))
            else:
                tot['other'] += 1
                P('   only in %-3s: class %d score %.6f: suppressed on the other side (IoU %.4f) by the row of score %.6f, kept here as well with IoU %.4f   <-- unexplained' % (side, c, r[26], float(iou_y.max()), K[26], iou_x))
P('\nrows matched by their nine points %d: max point difference %.3g px, max score difference %.3g; min-area-rect corners: max difference %.3g px but for %d rows' % (tot['matched'], worst_c, worst_s, worst_r, len(rect_flips)))
for c, sc, cd, pd in rect_flips:
    P('   class %d score %.6f: the nine points agree to %.3g px, the four corners differ by %.3g px: another rectangle / corner order of the same point set (a min-area-rect tie)' % (c, sc, pd, cd))
P('unmatched rows by cause: score threshold %d, IoU across the NMS threshold on the offset coordinates of the two sides %d, nms_pre top-k %d, suppressor has another min-area-rect %d, following from another flip %d, unexplained %d' % (tot['thr'], tot['nms'], tot['topk'], tot['rect'], tot['cascade'], tot['other']))
for name, rows_ in (('off', off['final']), ('on', on['final'])) if os.environ.get('OUT') else ():      # OUT=DIR: keep the rows
    np.savez(os.path.join(os.environ['OUT'], 'explain_rows_' + name + '.npz'), *[np.asarray(a) for a in rows_])

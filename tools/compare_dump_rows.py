"""Rows of two `bench.py --dump-outputs` directories (A: ORP_BN_DOWNSAMPLE_CONV_FUSE=0, B: on) matched per class by their nine points,
and every row that only one side has traced to the kept row that suppresses it on the other side.

    python tools/compare_dump_rows.py A B        (CPU only; needs the oracle library)

The NMS of `multiclass_rnms` runs on fp32 corners + label x (largest candidate coordinate + 1).  The dumps hold the kept rows only, so
each side's offset is taken from its largest KEPT coordinate; tests/checks/explain_dump_rows.py prints the largest candidate
coordinate of the same model and image, which is that row's.  IoUs are the oracle's quadrilateral IoU on the offset fp32 corners,
each side with its own offset."""
import glob, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import orp_oracle as O
A, B = sys.argv[1], sys.argv[2]
IOU = 0.4
q32 = lambda v: np.ascontiguousarray(v, dtype=np.float32)
files = sorted(os.path.basename(x) for x in glob.glob(A + '/*.npy'))
MAXC = {d: np.float32(max(float(np.load(os.path.join(d, f))[:, 18:26].max()) for f in files if len(np.load(os.path.join(d, f))))) for d in (A, B)}
print('largest kept coordinate: A %r, B %r: the class offsets differ by label x %.3g' % (float(MAXC[A]), float(MAXC[B]), abs(float(MAXC[A]) - float(MAXC[B]))))


def iou(c, mx, r, ks, plain=False):
    off = np.float32(0) if plain else np.float32(c) * (np.float32(mx) + np.float32(1))
    return O.quad_iou_matrix(q32(q32(r[None, 18:26]) + off), q32(q32(ks[:, 18:26]) + off))[0]


tot = dict(rows_a=0, rows_b=0, matched=0, rect_ties=0, offset=0, edge=0, by_rect=0, cascade=0, unexplained=0)
wp = ws = wr = 0.0
for c, f in enumerate(files):
    a, b = np.load(os.path.join(A, f)).astype(np.float64), np.load(os.path.join(B, f)).astype(np.float64)
    d = np.abs(a[:, None, :18] - b[None, :, :18]).max(-1)
    ma, mb, j = d.min(1) < 0.05, d.min(0) < 0.05, d.argmin(1)
    cd = np.abs(a[ma][:, 18:26] - b[j[ma]][:, 18:26]).max(1)
    wp = max(wp, float(np.abs(a[ma][:, :18] - b[j[ma]][:, :18]).max())); ws = max(ws, float(np.abs(a[ma][:, 26] - b[j[ma]][:, 26]).max()))
    wr = max(wr, float(cd[cd < 0.05].max()))
    print('%s: %3d / %3d rows, %3d matched by their nine points, %d of them with other min-area-rect corners, %d / %d on one side only'
          % (f, len(a), len(b), int(ma.sum()), int((cd >= 0.05).sum()), int((~ma).sum()), int((~mb).sum())), flush=True)
    for q in np.nonzero(cd >= 0.05)[0]:
        print('   tie: score %.6f, the nine points agree to %.3g px, the four corners are %.3g px apart: another rectangle of the same point set'
              % (a[ma][q, 26], float(np.abs(a[ma][q, :18] - b[j[ma]][q, :18]).max()), cd[q]))
    tot['rows_a'] += len(a); tot['rows_b'] += len(b); tot['matched'] += int(ma.sum()); tot['rect_ties'] += int((cd >= 0.05).sum())
    for side, rows, other, mask, mx_x, mx_y in (('A', a, b, ma, MAXC[A], MAXC[B]), ('B', b, a, mb, MAXC[B], MAXC[A])):
        for r in rows[~mask]:
            # kept on this side (X), not on the other (Y): which kept row of Y outranks and overlaps it there?
            hi = other[other[:, 26] > r[26] - 2e-7]
            iou_y = iou(c, mx_y, r, hi) if len(hi) else np.zeros(1)
            if iou_y.max() <= IOU:
                tot['unexplained'] += 1
                print('   only %s: score %.6f: no kept row of the other side overlaps it by more than %.1f at the other side\'s offset (largest IoU %.4f)   <-- unexplained'
                      % (side, r[26], IOU, iou_y.max()))
                continue
            K = hi[int(iou_y.argmax())]
            dk = np.abs(rows[:, :18] - K[None, :18]).max(1)
            if dk.min() >= 0.05:
                tot['cascade'] += 1
                print('   only %s: score %.6f: suppressed on the other side (IoU %.4f) by the row of score %.6f, which only the other side has: follows from that row'
                      % (side, r[26], iou_y.max(), K[26]))
                continue
            Kx = rows[int(dk.argmin())]
            cdk = float(np.abs(Kx[18:26] - K[18:26]).max())
            iou_x, plain = float(iou(c, mx_x, r, Kx[None])[0]), float(iou(c, 0, r, Kx[None], plain=True)[0])
            if cdk >= 0.05:
                tot['by_rect'] += 1
                print('   only %s: score %.6f: suppressed on the other side (IoU %.4f) by the row of score %.6f, whose min-area-rect is another rectangle there (corners %.3g px apart: a tie above); here the IoU is %.4f'
                      % (side, r[26], iou_y.max(), K[26], cdk, iou_x))
            elif iou_x <= IOU and mx_x != mx_y:
                tot['offset'] += 1
                print('   only %s: score %.6f against the kept row of score %.6f: IoU %.4f <= %.1f at this side\'s offset %d x (%.4f + 1), %.4f > %.1f at the other side\'s %d x (%.4f + 1); on the plain corners %.4f'
                      % (side, r[26], K[26], iou_x, IOU, c, float(mx_x), iou_y.max(), IOU, c, float(mx_y), plain))
            elif iou_x <= IOU:
                tot['edge'] += 1
                print('   only %s: score %.6f against the kept row of score %.6f: IoU %.6f here, %.6f on the other side: the NMS threshold %.1f' % (side, r[26], K[26], iou_x, iou_y.max(), IOU))
            else:
                tot['unexplained'] += 1
                print('   only %s: score %.6f: suppressed on the other side (IoU %.4f) by the row of score %.6f, kept here as well with IoU %.4f   <-- unexplained'
                      % (side, r[26], iou_y.max(), K[26], iou_x))
print('rows %d / %d; %d matched by their nine points: max point difference %.3g px (%.2g of the 1024 scale), max score difference %.3g, corners %.3g px apart but for %d min-area-rect ties'
      % (tot['rows_a'], tot['rows_b'], tot['matched'], wp, wp / 1024, ws, wr, tot['rect_ties']))
print('rows on one side only, by cause: IoU on either side of the NMS threshold at the two sides\' class offsets %d, at the threshold with equal offsets %d, suppressor has another min-area-rect %d, follows from another one-sided row %d, unexplained %d'
      % (tot['offset'], tot['edge'], tot['by_rect'], tot['cascade'], tot['unexplained']))

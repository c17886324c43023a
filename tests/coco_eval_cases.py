"""CPU helpers of the COCO-evaluation tests: a literal NumPy / Python restatement of pycocotools' COCOeval for boxes (computeIoU / evaluateImg / accumulate /
summarize, cocoeval.py and common/maskApi.c bbIou) written as the loops they are, with no vectorising cleverness -- the yardstick of the device path where
pycocotools is not installed -- and the seeded case generators.  tests/golden/make_coco_eval_golden.py records the restatement's arrays (and asserts equality with
pycocotools where it imports)."""
import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
P1 = 1 / (1 + 2.220446049250313e-16)   # a precision of "all true positives": tp / (0 + tp + spacing(1)) for tp = 1


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------------------
def box_iou(d, g, crowd):
    """bbIou of maskApi.c for one pair of [x, y, w, h] boxes"""
    w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    u = d[2] * d[3] if crowd else d[2] * d[3] + g[2] * g[3] - i
    return i / u


def evaluate_img(gts, dts, a_rng, max_det, iou_thrs):
    """evaluateImg for the ground truths and detections of ONE (image, category) pair, in file / arrival order.  gts: dicts with bbox, area, iscrowd; dts: dicts with
    bbox, score.  None when both are empty, else dict(dtm bool (T, D), dtIg bool (T, D), scores (D,), npig)."""
    if len(gts) == 0 and len(dts) == 0:
        return None
    g_ig = [1 if (g["iscrowd"] or g["area"] < a_rng[0] or g["area"] > a_rng[1]) else 0 for g in gts]
    gtind = np.argsort(g_ig, kind="mergesort")
    gt = [gts[i] for i in gtind]
    g_ig = [g_ig[i] for i in gtind]
    dtind = np.argsort([-d["score"] for d in dts], kind="mergesort")
    dt = [dts[i] for i in dtind[:max_det]]
    iscrowd = [int(g["iscrowd"]) for g in gt]
    ious = [[box_iou(d["bbox"], g["bbox"], c) for g, c in zip(gt, iscrowd)] for d in dt]
    T, G, D = len(iou_thrs), len(gt), len(dt)
    gtm = np.zeros((T, G), dtype=bool)
    dtm = np.zeros((T, D), dtype=bool)
    dt_ig = np.zeros((T, D), dtype=bool)
    if G and D:
        for tind, t in enumerate(iou_thrs):
            for dind in range(D):
                iou = min([t, 1 - 1e-10])
                m = -1
                for gind in range(G):
                    if gtm[tind, gind] and not iscrowd[gind]:
                        continue
                    if m > -1 and g_ig[m] == 0 and g_ig[gind] == 1:
                        break
                    if ious[dind][gind] < iou:
                        continue
                    iou = ious[dind][gind]
                    m = gind
                if m == -1:
                    continue
                dt_ig[tind, dind] = g_ig[m]
                dtm[tind, dind] = True
                gtm[tind, m] = True
    for dind, d in enumerate(dt):
        area = d["bbox"][2] * d["bbox"][3]
        if area < a_rng[0] or area > a_rng[1]:
            for tind in range(T):
                if not dtm[tind, dind]:
                    dt_ig[tind, dind] = True
    return dict(dtm=dtm, dtIg=dt_ig, scores=[d["score"] for d in dt], npig=sum(1 for x in g_ig if x == 0))


def _by_pair(items, img_ids, cat_ids):
    out = {}
    imgs, cats = set(img_ids), set(cat_ids)
    for it in items:
        if it["image_id"] in imgs and it["category_id"] in cats:
            out.setdefault((it["image_id"], it["category_id"]), []).append(it)
    return out


def coco_eval(anno, dets, img_ids=None, iou_thrs=None, rec_thrs=None, max_dets=None, area_rng=None):
    """COCOeval(gt, dt, "bbox").evaluate() + accumulate() -> (precision (T, R, K, A, M), recall (T, K, A, M), scores (T, R, K, A, M)).  anno: the annotation dict;
    dets: a list of {"image_id", "category_id", "bbox", "score"}."""
    iou_thrs = IOU_THRS if iou_thrs is None else np.asarray(iou_thrs, dtype=np.float64)
    rec_thrs = REC_THRS if rec_thrs is None else np.asarray(rec_thrs, dtype=np.float64)
    max_dets = MAX_DETS if max_dets is None else list(max_dets)
    area_rng = AREA_RNG if area_rng is None else area_rng
    img_ids = sorted(set(im["id"] for im in anno["images"])) if img_ids is None else sorted(set(img_ids))
    cat_ids = sorted(set(c["id"] for c in anno["categories"]))
    gts = _by_pair([dict(g, iscrowd=int(g.get("iscrowd", 0))) for g in anno["annotations"]], img_ids, cat_ids)
    dts = _by_pair(dets, img_ids, cat_ids)
    T, R, K, A, M = len(iou_thrs), len(rec_thrs), len(cat_ids), len(area_rng), len(max_dets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    for k, cat in enumerate(cat_ids):
        for a, rng in enumerate(area_rng):
            E = [evaluate_img(gts.get((img, cat), []), dts.get((img, cat), []), rng, max_dets[-1], iou_thrs) for img in img_ids]
            E = [e for e in E if e is not None]
            if len(E) == 0:
                continue
            npig = sum(e["npig"] for e in E)
            if npig == 0:
                continue
            for m, max_det in enumerate(max_dets):
                dt_scores = np.concatenate([np.asarray(e["scores"][0:max_det], dtype=np.float64) for e in E])
                inds = np.argsort(-dt_scores, kind="mergesort")
                sorted_scores = dt_scores[inds]
                dtm = np.concatenate([e["dtm"][:, 0:max_det] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e["dtIg"][:, 0:max_det] for e in E], axis=1)[:, inds]
                for t in range(T):
                    tp_run, fp_run, rc, pr = 0, 0, [], []
                    for j in range(len(sorted_scores)):
                        tp_run += 1 if (dtm[t, j] and not dt_ig[t, j]) else 0
                        fp_run += 1 if (not dtm[t, j] and not dt_ig[t, j]) else 0
                        tp, fp = float(tp_run), float(fp_run)
                        rc.append(tp / npig)
                        pr.append(tp / (fp + tp + np.spacing(1)))
                    recall[t, k, a, m] = rc[-1] if rc else 0
                    for i in range(len(pr) - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    q, ss = np.zeros(R), np.zeros(R)
                    for ri, r in enumerate(rec_thrs):
                        pi = 0
                        while pi < len(rc) and rc[pi] < r:   # searchsorted(rc, r, side="left")
                            pi += 1
                        if pi >= len(rc):
                            break
                        q[ri] = pr[pi]
                        ss[ri] = sorted_scores[pi]
                    precision[t, :, k, a, m] = q
                    scores[t, :, k, a, m] = ss
    return precision, recall, scores


_ROWS = [(1, None, "all", -1), (1, .5, "all", -1), (1, .75, "all", -1), (1, None, "small", -1), (1, None, "medium", -1), (1, None, "large", -1),
         (0, None, "all", 0), (0, None, "all", 1), (0, None, "all", 2), (0, None, "small", -1), (0, None, "medium", -1), (0, None, "large", -1)]
_AREA_NAMES = ["all", "small", "medium", "large"]


def summarize(precision, recall, iou_thrs=None, max_dets=None):
    """the twelve numbers of COCOeval.summarize and its twelve lines"""
    iou_thrs = IOU_THRS if iou_thrs is None else np.asarray(iou_thrs)
    max_dets = MAX_DETS if max_dets is None else list(max_dets)
    stats, lines = [], []
    for ap, iou, area, mi in _ROWS:
        a, m = _AREA_NAMES.index(area), (len(max_dets) + mi if mi < 0 else mi)
        s = precision[:, :, :, a, m] if ap else recall[:, :, a, m]
        if iou is not None:
            s = s[np.where(iou == iou_thrs)[0]]
        mean = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        stats.append(mean)
        iou_str = "{:0.2f}:{:0.2f}".format(iou_thrs[0], iou_thrs[-1]) if iou is None else "{:0.2f}".format(iou)
        lines.append(" {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}".format(
            "Average Precision" if ap else "Average Recall", "(AP)" if ap else "(AR)", iou_str, area, max_dets[m], mean))
    return np.array(stats), lines


def evaluate(anno, dets, img_ids=None):
    p, r, s = coco_eval(anno, dets, img_ids)
    return dict(precision=p, recall=r, scores=s, stats=summarize(p, r)[0])


# ---- cases worked by hand ------------------------------------------------------------------------------------------------------------------------------------------
def _anno(gts, n_img=1, cats=(1,)):
    return dict(images=[dict(id=i + 1) for i in range(n_img)], categories=[dict(id=c) for c in cats],
                annotations=[dict(id=i + 1, image_id=g[0], category_id=g[1], bbox=list(g[2]), area=g[3], iscrowd=g[4]) for i, g in enumerate(gts)])


def _det(img, cat, box, score):
    return dict(image_id=img, category_id=cat, bbox=list(box), score=score)


def hand_case(name):
    """(annotation dict, detections, the stats worked by hand)"""
    p = P1
    box = [10, 10, 50, 40]
    if name == "A":
        return _anno([(1, 1, box, 2000, 0)]), [_det(1, 1, box, 0.9)], [p, p, p, -1, p, -1, 1, 1, 1, -1, 1, -1]
    if name == "B":
        return _anno([(1, 1, box, 2000, 0)]), [_det(1, 1, [200, 200, 50, 40], 0.9), _det(1, 1, box, 0.8)], [.5, .5, .5, -1, .5, -1, 0, 1, 1, -1, 1, -1]
    if name == "C":
        anno = _anno([(1, 1, [0, 0, 100, 100], 10000, 1), (1, 1, [200, 200, 30, 30], 900, 0)])
        dets = [_det(1, 1, [10, 10, 20, 20], 0.9), _det(1, 1, [50, 50, 20, 20], 0.8), _det(1, 1, [200, 200, 30, 30], 0.7)]
        return anno, dets, [p, p, p, p, -1, -1, 0, 1, 1, 1, -1, -1]
    raise KeyError(name)


# ---- seeded scenes ---------------------------------------------------------------------------------------------------------------------------------------------------
SCENES = {"mixed": 11, "crowded": 12, "ties": 13}
N_IMG, CATS = 6, (1, 3, 7)          # image ids 101 .. 106 (+ 107, which has no annotation); category 9 is in `categories` without annotations, 5 is in neither
BIG_G = 300                         # ground truths of the largest pair


def scene(name):
    """-> (annotation dict, detections, img_ids or None).  Every scene holds: a pair with 130 detections and one with BIG_G ground truths; duplicated scores inside a
    pair and across images; crowds that several detections match; areas on the 32^2 and 96^2 boundaries; images with detections and no ground truth and the reverse; a
    category without ground truth; a detection category outside the file; detections of an image left out of img_ids ("crowded", "ties")."""
    rng = np.random.default_rng(SCENES[name])
    imgs = list(range(101, 101 + N_IMG + 1))
    gts, dets = [], []

    def rbox(lo=4, hi=120):
        w, h = rng.integers(lo, hi, 2)
        x, y = rng.integers(0, 400, 2)
        return [float(x), float(y), float(w), float(h)]

    def jitter(b, s):
        return [round(float(v + rng.normal(0, s)), 3) for v in b[:2]] + [round(float(max(v + rng.normal(0, s), 1.0)), 3) for v in b[2:]]

    def score():
        return round(float(rng.integers(1, 40)) / 40, 5) if name == "ties" else round(float(rng.random()), 5)   # "ties": 39 values only

    for img in imgs[:N_IMG]:
        for cat in CATS:
            if (img, cat) in ((102, 3), (104, 1), (104, 3), (104, 7)):   # image 104: detections, no ground truth
                continue
            for _ in range(int(rng.integers(1, 6))):
                b = rbox()
                crowd = int(rng.random() < (0.4 if name == "crowded" else 0.15))
                if crowd:
                    b = [b[0], b[1], b[2] * 2, b[3] * 2]
                area = b[2] * b[3] * float(rng.choice([1.0, 1.0, 0.6]))   # the annotation's area is not w * h
                gts.append((img, cat, b, area, crowd))
    gts.append((101, 1, [5.0, 5.0, 32.0, 32.0], 1024.0, 0))       # exactly 32^2: small and medium
    gts.append((101, 1, [60.0, 60.0, 96.0, 96.0], 9216.0, 0))     # exactly 96^2: medium and large
    gts.append((103, 7, [0.0, 0.0, 300.0, 300.0], 90000.0, 1))    # one crowd under many detections
    for _ in range(BIG_G):                                          # the largest pair
        gts.append((105, 3, rbox(4, 40), float(rng.integers(100, 12000)), int(rng.random() < 0.05)))
    order = rng.permutation(len(gts))                               # file order is not grouped
    gts = [gts[i] for i in order]
    for g in gts:
        if g[0] == 106:                                             # image 106: ground truth, no detections
            continue
        for _ in range(int(rng.integers(0, 4))):
            dets.append(_det(g[0], g[1], jitter(g[2], float(rng.choice([0.5, 3.0, 10.0]))), score()))
    for _ in range(130):                                            # crosses the cap of 100 and maxDets 1 / 10
        dets.append(_det(103, 7, rbox(4, 60), score()))
    for img in (104, 107):
        for _ in range(12):
            dets.append(_det(img, int(rng.choice(CATS)), rbox(), score()))
    for _ in range(8):
        dets.append(_det(101, 9, rbox(), score()))                  # a category without ground truth
        dets.append(_det(102, 5, rbox(), score()))                  # a category outside the file
    dets.append(_det(101, 1, [5.0, 5.0, 32.0, 32.0], 0.99))
    dets.append(_det(101, 1, [60.0, 60.0, 96.0, 96.0], 0.99))      # the same score twice in one pair
    dets.append(_det(102, 1, rbox(), 0.99))                         # ... and in another image
    dets = [dets[i] for i in rng.permutation(len(dets))]
    anno = dict(images=[dict(id=i, file_name=f"{i:012d}.jpg") for i in imgs], categories=[dict(id=c, name=str(c)) for c in (*CATS, 9)],
                annotations=[dict(id=i + 1, image_id=g[0], category_id=g[1], bbox=g[2], area=g[3], iscrowd=g[4]) for i, g in enumerate(gts)])
    for a in anno["annotations"][::7]:
        del a["iscrowd"]                                            # a missing field counts as 0
    for a in anno["annotations"][::5]:
        a["ignore"] = 1                                             # overwritten by iscrowd, as pycocotools does
    img_ids = None if name == "mixed" else [101, 102, 103, 104, 106, 107, 103]   # 105 left out (its detections take no part); a duplicate
    return anno, dets, img_ids


def dets_array(dets):
    """the (N, 7) form [image_id, category_id, x, y, w, h, score]"""
    return np.array([[d["image_id"], d["category_id"], *d["bbox"], d["score"]] for d in dets], dtype=np.float64).reshape(-1, 7)


def fixture_scene():
    """the small scene tests/golden/coco_eval.pt records whole: 3 images x 2 categories with a crowd, both area boundaries, a score tie across images, an image
    without ground truth and one without detections -> (annotation dict, detections)"""
    rng = np.random.default_rng(7)
    gts = [(1, 1, [5.0, 5.0, 32.0, 32.0], 1024.0, 0), (1, 1, [60.0, 60.0, 96.0, 96.0], 9216.0, 0), (1, 2, [0.0, 0.0, 200.0, 150.0], 30000.0, 1),
           (2, 2, [30.0, 40.0, 50.0, 60.0], 2400.5, 0), (2, 1, [100.0, 100.0, 20.0, 10.0], 150.0, 0), (1, 2, [20.0, 30.0, 40.0, 40.0], 1500.0, 0)]
    for _ in range(10):
        w, h = rng.integers(6, 110, 2)
        gts.append((int(rng.integers(1, 3)), int(rng.integers(1, 3)), [float(rng.integers(0, 300)), float(rng.integers(0, 300)), float(w), float(h)], float(w * h) * 0.8, 0))
    dets = []
    for g in gts:
        for s in (1.0, 6.0):
            b = [round(float(v + rng.normal(0, s)), 3) for v in g[2]]
            dets.append(_det(g[0], g[1], [b[0], b[1], max(b[2], 1.0), max(b[3], 1.0)], round(float(rng.integers(1, 30)) / 30, 5)))
    for _ in range(15):
        dets.append(_det(3, int(rng.integers(1, 3)), [float(rng.integers(0, 300)), float(rng.integers(0, 300)), 30.0, 30.0], round(float(rng.random()), 5)))   # image 3: no ground truth
        dets.append(_det(1, 2, [float(rng.integers(0, 180)), float(rng.integers(0, 130)), 15.0, 15.0], round(float(rng.random()), 5)))                     # under the crowd
    anno = dict(images=[dict(id=i) for i in (1, 2, 3, 4)], categories=[dict(id=1, name="a"), dict(id=2, name="b")],
                annotations=[dict(id=i + 1, image_id=g[0], category_id=g[1], bbox=g[2], area=g[3], iscrowd=g[4]) for i, g in enumerate(gts)])
    anno["annotations"].append(dict(id=len(gts) + 1, image_id=4, category_id=1, bbox=[10.0, 10.0, 40.0, 40.0], area=1600.0, iscrowd=0))   # image 4: no detections
    return anno, dets


def long_scene():
    """30 images x 2 categories, 45 detections per pair: more than 1024 rows in one category (the accumulate kernel's chunk), scores on a grid of 50 values ->
    (annotation dict, detections)"""
    rng = np.random.default_rng(21)
    gts, dets = [], []
    for img in range(1, 31):
        for cat in (1, 2):
            mine = []
            for _ in range(int(rng.integers(1, 5))):
                w, h = rng.integers(10, 120, 2)
                mine.append([float(rng.integers(0, 300)), float(rng.integers(0, 300)), float(w), float(h)])
                gts.append((img, cat, mine[-1], float(w * h), int(rng.random() < 0.1)))
            for j in range(45):
                b = mine[j % len(mine)] if j < 12 else [float(rng.integers(0, 300)), float(rng.integers(0, 300)), 40.0, 40.0]
                s = float(rng.choice([1.0, 4.0, 12.0]))
                b = [round(float(v + rng.normal(0, s)), 3) for v in b]
                dets.append(_det(img, cat, [b[0], b[1], max(b[2], 1.0), max(b[3], 1.0)], round(float(rng.integers(1, 51)) / 50, 5)))
    dets = [dets[i] for i in rng.permutation(len(dets))]
    return _anno(gts, n_img=30, cats=(1, 2)), dets

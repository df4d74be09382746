"""The inputs of ``test_head_ref_cpu.py`` and ``test_head_kernels_fp64_gpu.py``: seeded, float32, in the
kernels' layouts, and built so that every piecewise-constant choice a kernel makes is DECIDED -- an
exact tie of float32 values or a gap no rounding can close (``test_head_ref_cpu.py`` proves it):

* centres of proposals and boxes on a 1/4 lattice in [-2, 2]^3 (a sub-lattice of 1/64): squared
  distances are multiples of 1/16 below 48, exact in float32, equal or >= 1/768 apart;
* logits on a 1/8 grid (to +-80): equal or >= 1/640 apart;
* planes and their targets on a 1/64 lattice: |error| is 1/4 exactly or >= 1/16 away from it;
* votes, seeds and vote targets on a 1/64 lattice: L1 distances below 12, equal or >= 1/768 apart,
  a residual is 0 or at least 1/64;
* headings whose sin / cos difference is not within 2^-9 of beta (moved onto the target: difference 0).
"""
import functools
import itertools

import torch

from tests import _head_ref as R

HEAD_SHAPES = [(1, 1, 1, 1), (2, 32, 4, 18), (2, 64, 1, 18), (3, 70, 5, 18), (5, 130, 9, 32),
               (8, 256, 64, 18)]
ALL_FORMS_AT = [(3, 70, 5, 18), (8, 256, 64, 18)]
REGIMES = ('benign', 'saturated', 'ties', 'weights')
FORMS = dict(sup0=dict(sigma_mode=0), sup1=dict(sigma_mode=1), sup2=dict(sigma_mode=2),
             label=dict(sigma_mode=0, label=True), unsup=dict(unsup=True, detach_sigma=False),
             unsup_detach=dict(unsup=True, detach_sigma=True))
# alpha, objectness weight and class weights, semantic, chamfer source / destination, surface, iou,
# iou_pred, side: the shipped values except where two would be equal (a swap must show)
CONFIG = [0.5, 5.0, 0.2, 0.8, 1.0, 10.0, 7.0, 10.0, 3.0, 2.5, 1.5]
# objectness weight and class weights, angle weight, SmoothL1 beta, angle-quality weight, side weight
SAQE_CONFIG = [5.0, 0.2, 0.8, 10.0, 0.5, 1.25, 1.5]
G7 = ([0.7, -1.3, 0.9, 1.1, 0.0, 1.2, -0.6], [0.0, 1.0, -0.5, 0.3, 2.0, -1.5, 0.25])
G4 = ([0.7, -1.3, 0.0, 1.1], [0.0, 0.5, -0.9, 0.4])


def forms_of(shape):
    return list(FORMS) if shape in ALL_FORMS_AT else ['sup0', 'unsup']


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(v) for i, v in enumerate(key)) % (2 ** 31))


def _lattice(g, shape, lo, hi, step):
    return torch.randint(int(lo * step), int(hi * step) + 1, shape, generator=g).float() / step


def _logits(g, shape, regime):
    if regime == 'saturated':
        return _lattice(g, shape, -80, 80, 8)
    return torch.round(torch.randn(shape, generator=g) * 16) / 8


def _probs(g, shape, regime):
    p = torch.rand(shape, generator=g) * 0.96 + 0.02
    if regime == 'saturated':
        edge = torch.tensor([0.0, 1.0, 1e-30, 1.0 - 2.0 ** -24])
        which = torch.randint(0, 6, shape, generator=g)
        p = torch.where(which < 4, edge[which.clamp_max(3)], p)
    return p


def _ious(g, n, regime):
    v = torch.rand(n, generator=g)
    if regime == 'saturated':
        which = torch.randint(0, 3, (n,), generator=g)
        v = torch.where(which == 0, torch.zeros(n), torch.where(which == 1, torch.ones(n), v))
    return v


@functools.lru_cache(maxsize=None)
def head_case(shape, regime):
    """-> dict(x = the predictions, tg = the targets, quality, iou_label, saqe = the extras' inputs)."""
    B, K, Tn, C = shape
    g = _gen(B, K, Tn, C, REGIMES.index(regime))
    N = B * K
    gt_c = _lattice(g, (B, Tn, 3), -2, 2, 4)
    gt_size = _lattice(g, (B, Tn, 3), 1 / 32, 2, 32)
    gt_yaw = torch.rand(B, Tn, generator=g) * 6 - 3
    gt_label = torch.randint(0, C, (B, Tn), generator=g)
    count = torch.tensor([Tn]) if B == 1 else torch.round(torch.linspace(0, Tn, B)).long()
    centre = _lattice(g, (B, K, 3), -2, 2, 4)
    if regime == 'ties':
        # two proposals equidistant from every box centre, two box centres equidistant from every
        # proposal (first minimum decides), and boxes sharing their nearest proposal
        centre[:, 1::4] = centre[:, 0:K - 1:4][:, :centre[:, 1::4].shape[1]]
        gt_c[:, 1::2] = gt_c[:, 0:Tn - 1:2][:, :gt_c[:, 1::2].shape[1]]
        if K > 1:
            centre[:, 0] = centre[:, 1] = gt_c[:, 0]
    col = torch.arange(Tn)[None, :] < count[:, None]
    assign = (torch.rand(B, K, generator=g) * count.clamp_min(1)[:, None]).long()
    take = lambda t: torch.gather(t, 1, assign.unsqueeze(-1).expand(B, K, t.shape[-1]))  # noqa: E731
    bbox_t = torch.cat([take(gt_c), take(gt_size), take(gt_yaw.unsqueeze(-1))], -1)
    label = torch.gather(gt_label, 1, assign)

    pos = torch.rand(B, K, generator=g) < 0.5
    neg = ~pos & (torch.rand(B, K, generator=g) < 0.5)
    if regime == 'weights':
        pos[0], neg[0] = False, True
        if B > 1:
            pos[1], neg[1] = True, False
    if not pos.any():
        pos[-1, -1], neg[-1, -1] = True, False
    obj_w = (pos | neg).float() / ((pos | neg).sum().float() + 1e-6)
    box_w = pos.float() / (pos.sum().float() + 1e-6)
    valid = col.float()
    tg = dict(obj_targets=pos.long(), mask_targets=label, obj_weights=obj_w, box_weights=box_w,
              bbox_targets=bbox_t, center_targets=torch.where(col.unsqueeze(-1), gt_c, torch.zeros(())),
              valid_weights=valid / (valid.sum() + 1e-6))

    cls = _logits(g, (B, 2 + C, K), regime)
    if regime == 'ties' and C > 1:
        sem = cls[:, 2:]
        top = sem.max(1, keepdim=True).values
        other = torch.randint(0, C, (B, 1, K), generator=g)
        tie = torch.rand(B, 1, K, generator=g) < 0.5
        sem.scatter_(1, other, torch.where(tie, top, sem.gather(1, other)))
        # the assigned class is the arg-max class for about half of the proposals
        pick = sem.argmax(1)
        tg['mask_targets'] = torch.where(torch.rand(B, K, generator=g) < 0.5, pick, label)
    tb = bbox_t.reshape(N, 7)
    planes = torch.cat([tb[:, :3] - 0.5 * tb[:, 3:6], tb[:, :3] + 0.5 * tb[:, 3:6]], 1).reshape(B, K, 6)
    reach = 1 if regime == 'saturated' else 0.5
    surface = planes + _lattice(g, (B, K, 6), -reach, reach, 64)
    jsurf = planes + _lattice(g, (B, K, 6), -reach, reach, 64)
    # headings: a third on their target (difference 0), the rest anywhere (both sides of beta)
    yaw = torch.rand(B, K, generator=g) * 6 - 3
    yaw = torch.where(torch.rand(B, K, generator=g) < 1 / 3, bbox_t[..., 6], yaw)
    beta = SAQE_CONFIG[4]
    for f in (torch.sin, torch.cos):
        gap = ((f(yaw.double()) - f(bbox_t[..., 6].double())).abs() - beta).abs()
        yaw = torch.where(gap < 2.0 ** -9 * beta, bbox_t[..., 6], yaw)
    bbox = torch.cat([centre, torch.rand(B, K, 3, generator=g) + 0.1, yaw.unsqueeze(-1)], -1)
    x = dict(cls=cls, bbox=bbox, surface=surface, side=_probs(g, (6, B, C, 2 * K), regime),
             iou_s=_probs(g, (B, 2 * K, C), regime), iou=_ious(g, N, regime), iou_j=_ious(g, N, regime))
    quality = torch.rand(B, K, 6, generator=g) * 0.95 + 0.05
    dead = torch.rand(B, K, generator=g) < (0.3 if regime == 'weights' else 0.1)
    quality[dead] = 0.0
    saqe = dict(robj=_logits(g, (B, 2 * K, 2), regime).contiguous(), rot=_probs(g, (B, 2 * K, C), regime),
                bbox=bbox, bbox_t=bbox_t, jsurf=jsurf, side=x['side'])
    return dict(x=x, tg=tg, quality=quality.reshape(N, 6), iou_label=_ious(g, N, regime), saqe=saqe,
                count=count)


def head_kwargs(case, form):
    f = FORMS[form]
    if f.get('unsup'):
        return dict(quality=case['quality'], detach_sigma=f['detach_sigma'])
    return dict(sigma_mode=f['sigma_mode'], iou_label=case['iou_label'] if f.get('label') else None)


def head_run(shape, regime, form, gi, dtype):
    case = head_case(shape, regime)
    out = R.head_loss(R.cast(case['x'], dtype), case['tg'], CONFIG, g=G7[gi],
                      **R.cast(head_kwargs(case, form), dtype))
    return out


@functools.lru_cache(maxsize=None)
def head_ref(shape, regime, form, gi):
    """The float64 answer of a case (kept: the CPU measurement and the device tests share it)."""
    return head_run(shape, regime, form, gi, torch.float64)


def saqe_run(shape, regime, sup, gi, dtype):
    case = head_case(shape, regime)
    pick = head_ref(shape, regime, 'sup0', 0)['sem_pick']
    return R.saqe_extra(R.cast(case['saqe'], dtype), case['tg'], pick, SAQE_CONFIG, sup, g=G4[gi])


@functools.lru_cache(maxsize=None)
def saqe_ref(shape, regime, sup, gi):
    return saqe_run(shape, regime, sup, gi, torch.float64)


# ---- vote loss ------------------------------------------------------------------------------------------
VOTE_SIZES = {1: (1, 1), 255: (3, 85), 256: (2, 128), 257: (1, 257), 8192: (8, 1024), 16384: (8, 2048),
              17000: (8, 2125)}
VOTE_MASKS = ('mixed', 'ones', 'zeros')
VOTE_W, VOTE_G = 10.0, -0.75


@functools.lru_cache(maxsize=None)
def vote_case(bn, gps, mask_kind):
    b, n = VOTE_SIZES[bn]
    g = _gen(bn, gps, VOTE_MASKS.index(mask_kind), 3)
    npts = 2 * n + 3
    seed_idx = torch.randint(0, npts, (b, n), generator=g)
    mask = dict(mixed=(torch.rand(b, npts, generator=g) < 0.5).long(),
                ones=torch.ones(b, npts, dtype=torch.long),
                zeros=torch.zeros(b, npts, dtype=torch.long))[mask_kind]
    targets = _lattice(g, (b, npts, 3 * gps), -1, 1, 64)
    if gps > 1:      # equal targets: the first minimum
        same = torch.rand(b, npts, generator=g) < 0.5
        targets[..., 3:6] = torch.where(same.unsqueeze(-1), targets[..., 0:3], targets[..., 3:6])
    seed = _lattice(g, (b, n, 3), -1, 1, 64)
    vote = _lattice(g, (b, n, 3), -2, 2, 64)
    first = torch.gather(targets[..., :3], 1, seed_idx.unsqueeze(-1).expand(b, n, 3)) + seed
    hit = torch.rand(b, n, generator=g) < 0.1
    hit[0, 0] = bn > 1
    vote = torch.where(hit.unsqueeze(-1), first, vote)      # a vote exactly on its target
    return dict(seed=seed, vote=vote, seed_idx=seed_idx, mask=mask, targets=targets)


def vote_ref(bn, gps, mask_kind, dtype=torch.float64):
    c = R.cast(vote_case(bn, gps, mask_kind), dtype)
    return R.vote_loss(c['seed'], c['vote'], c['seed_idx'], c['mask'], c['targets'], VOTE_W, g=VOTE_G)


# ---- side decode ----------------------------------------------------------------------------------------
DECODE_K, DECODE_BINS, DECODE_B, DECODE_SPREAD = (1, 63, 64, 65, 200), (2, 17, 33), (1, 3), (2, 60)
DECODE_GRADS = ('surface', 'bbox', 'both')


@functools.lru_cache(maxsize=None)
def decode_case(b, k, bins, spread):
    g = _gen(b, k, bins, spread, 5)
    reg = torch.randn(b, 6 * bins + 2, k, generator=g) * 2 if spread == 2 else \
        (torch.rand(b, 6 * bins + 2, k, generator=g) * 2 - 1) * spread
    # heading pairs in all four quadrants, every fourth with h1 < 0 and a small |h0| of either sign
    mag = torch.rand(b, 2, k, generator=g) * 1.9 + 0.1
    sgn = torch.randint(0, 2, (b, 2, k), generator=g).float() * 2 - 1
    h = mag * sgn
    h[:, 0, 0::4] = sgn[:, 0, 0::4] * 1e-3 * mag[:, 0, 0::4]
    h[:, 1, 0::4] = -mag[:, 1, 0::4]
    reg[:, 6 * bins:] = h
    return dict(reg=reg.contiguous(), agg=torch.randn(b, k, 3, generator=g),
                scale=torch.tensor([3.0, 3.0, 2.5, 3.0, 3.0, 2.5]),
                sign=torch.tensor([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]),
                d_surface=torch.randn(b, k, 6, generator=g), d_bbox=torch.randn(b, k, 7, generator=g))


def decode_ref(b, k, bins, spread, grads, dtype=torch.float64):
    c = R.cast(decode_case(b, k, bins, spread), dtype)
    return R.side_decode(c['reg'], c['agg'], c['scale'], c['sign'],
                         c['d_surface'] if grads in ('surface', 'both') else None,
                         c['d_bbox'] if grads in ('bbox', 'both') else None)


# ---- vote finish ----------------------------------------------------------------------------------------
FINISH_C, FINISH_N, FINISH_B = (1, 3, 4, 5, 256), (1, 63, 64, 65, 1024), 2
FINISH_GRADS = ('both', 'feats', 'points')


@functools.lru_cache(maxsize=None)
def finish_case(c, n):
    g = _gen(c, n, 11)
    b = FINISH_B
    return dict(raw=torch.randn(b, 3 + c, n, generator=g), seed_points=torch.randn(b, n, 3, generator=g),
                seed_feats=torch.randn(b, c, n, generator=g), g_feats=torch.randn(b, c, n, generator=g),
                g_points=torch.randn(b, n, 3, generator=g))


def finish_ref(c, n, normalise, grads, dtype=torch.float64):
    k = R.cast(finish_case(c, n), dtype)
    return R.vote_finish(k['raw'], k['seed_points'], k['seed_feats'], normalise,
                         k['g_feats'] if grads in ('both', 'feats') else None,
                         k['g_points'] if grads in ('both', 'points') else None, backward=True)


# ---- the float32 referee against the float64 referee -------------------------------------------------
def head_cases():
    return [(s, r) for s in HEAD_SHAPES for r in REGIMES]


FAMILIES = ('head', 'vote', 'decode', 'finish')


def float32_ratios():
    """{output: worst float32-referee error / (2^-24 S)} over every case above."""
    return {k: v for f in FAMILIES for k, v in family_ratios(f).items()}


@functools.lru_cache(maxsize=None)
def family_ratios(family):
    worst = {}

    def note(name, got, want):
        worst[name] = max(worst.get(name, 0.0), R.ratio(got.v, want))

    for shape, regime in head_cases() if family == 'head' else ():
        for form, gi in itertools.product(forms_of(shape), range(len(G7))):
            a, b = head_run(shape, regime, form, gi, torch.float32), head_ref(shape, regime, form, gi)
            assert torch.equal(a['sem_pick'], b['sem_pick']) and torch.equal(a['kstar'], b['kstar'])
            note('head.terms', a['terms'], b['terms'])
            for k in a['grads']:
                note('head.d_' + k, a['grads'][k], b['grads'][k])
        for sup, gi in itertools.product((0, 1), range(len(G4))):
            a, b = saqe_run(shape, regime, sup, gi, torch.float32), saqe_ref(shape, regime, sup, gi)
            note('saqe.terms', a['terms'], b['terms'])
            for k in a['grads']:
                note('saqe.d_' + k, a['grads'][k], b['grads'][k])
    for bn, gps, mk in itertools.product(VOTE_SIZES, (1, 3), VOTE_MASKS) if family == 'vote' else ():
        a, b = vote_ref(bn, gps, mk, torch.float32), vote_ref(bn, gps, mk)
        assert torch.equal(a['sign'].double(), b['sign'])
        for k in ('loss', 'scale', 'd_vote'):
            note('vote.' + k, a[k], b[k])
    for bb, k, bins, spread in itertools.product(DECODE_B, DECODE_K, DECODE_BINS, DECODE_SPREAD) \
            if family == 'decode' else ():
        for grads in DECODE_GRADS:
            a, b = decode_ref(bb, k, bins, spread, grads, torch.float32), decode_ref(bb, k, bins, spread, grads)
            for name in a:
                note('decode.' + name, a[name], b[name])
    for c, n, normalise, grads in itertools.product(FINISH_C, FINISH_N, (True, False), FINISH_GRADS) \
            if family == 'finish' else ():
        a, b = finish_ref(c, n, normalise, grads, torch.float32), finish_ref(c, n, normalise, grads)
        for name in a:
            note('finish.' + name, a[name], b[name])
    return worst


# ---- head targets ---------------------------------------------------------------------------------------
# (B, K, T): the training shape, 1500 proposals (a ragged second stride of the 1024 threads), 1170 boxes
TARGET_SHAPES = [(8, 256, 64), (5, 300, 7), (9, 40, 130)]
# the shipped thresholds; sqrt(d + 1e-6) of a lattice distance d = n / 16 is 0.001, 0.25, 0.354, ..,
# 0.559 | 0.612, ..: positive up to d = 1/16, ignored up to 5/16, negative from 6/16
POS_THR, NEG_THR = 0.3, 0.6


@functools.lru_cache(maxsize=None)
def target_case(shape):
    """-> agg (B,K,3) and the padded ground truth of ``GTBatch.collate`` (an empty scene first)."""
    from nesie_amd.votenet.nesie_head import GTBatch
    B, K, Tn = shape
    g = _gen(B, K, Tn, 17)
    counts = torch.round(torch.linspace(0, Tn, B)).long().tolist()
    boxes, labels = [], []
    for n in counts:
        height = _lattice(g, (n, 1), 0.5, 2, 2)                 # centre z = bottom + height / 2: on the lattice
        centre = _lattice(g, (n, 3), -2, 2, 4)
        boxes.append(torch.cat([centre[:, :2], centre[:, 2:] - 0.5 * height,
                                _lattice(g, (n, 2), 1 / 32, 2, 32), height,
                                torch.rand(n, 1, generator=g) * 6 - 3], -1))
        labels.append(torch.randint(0, 18, (n,), generator=g))
    gt = GTBatch.collate(boxes, labels, torch.device('cpu'))
    agg = _lattice(g, (B, K, 3), -2, 2, 4)
    for b, n in enumerate(counts):
        if n == 0:
            continue
        c = torch.cat([boxes[b][:, :2], (boxes[b][:, 2] + 0.5 * boxes[b][:, 5]).unsqueeze(-1)], -1)
        near = c[torch.randint(0, n, (K,), generator=g)]
        axis = torch.nn.functional.one_hot(torch.randint(0, 3, (K,), generator=g), 3).float()
        step = torch.randint(0, 2, (K, 1), generator=g).float() * 0.25
        agg[b, 0::3] = (near + axis * step)[0::3]               # on a centre or one step away: positive
        agg[b, 1::3] = (near + 0.25)[1::3]                      # d = 3/16 at most: ignored unless another box is nearer
    return dict(agg=agg, gt_boxes=gt.boxes, gt_labels=gt.labels, gt_count=gt.count, gt_valid=gt.valid,
                counts=counts)

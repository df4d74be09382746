"""``csrc/head_loss.hip``, ``csrc/decode.hip`` and ``csrc/vote.hip`` through ``HipKernels`` against the
float64 referee of ``tests/_head_ref.py`` on the inputs of ``tests/_head_cases.py``: every element
within c 2^-24 S + 2^-126, c = four times the float32 referee's own worst error on the same inputs
(``R.RECORDED``, re-measured by ``test_head_ref_cpu.py``; never taken from a kernel), no element
excused."""
import itertools
import types

import pytest
import torch

from tests import _head_cases as H
from tests import _head_ref as R

pytestmark = pytest.mark.gpu


def _dev(obj, device):
    if torch.is_tensor(obj):
        return obj.to(device).contiguous()
    if isinstance(obj, dict):
        return {k: _dev(v, device) for k, v in obj.items()}
    return obj


def _ticket(device):
    return torch.zeros(1, dtype=torch.int32, device=device)


def _head_forward(hip, x, tg, case, form, ticket):
    kw = H.head_kwargs(case, form)
    kw = {k: (v.to(ticket.device) if torch.is_tensor(v) else v) for k, v in kw.items()}
    return hip.head_loss_forward(x['cls'], x['bbox'], x['surface'], x['side'], x['iou_s'], x['iou'],
                                 x['iou_j'], tg, H.CONFIG, ticket, **kw)


def _same_bits(a, b):
    a, b = (list(t.values()) if isinstance(t, dict) else [t] for t in (a, b))
    return all(torch.equal(p.view(torch.int32) if p.dtype == torch.float32 else p,
                           q.view(torch.int32) if q.dtype == torch.float32 else q) for p, q in zip(a, b))


@pytest.mark.parametrize('regime', H.REGIMES)
@pytest.mark.parametrize('shape', H.HEAD_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_head_loss_against_float64(hip_device, shape, regime):
    from nesie_amd.kernels import backend_for
    c = R.constants()
    B, K, Tn, C = shape
    case = H.head_case(shape, regime)
    x, tg = _dev(case['x'], hip_device), _dev(case['tg'], hip_device)
    hip = backend_for(x['cls'])
    ticket = _ticket(hip_device)
    worst = {}
    for form in H.forms_of(shape):
        what = f'{shape} {regime} {form}'
        loss, sv = _head_forward(hip, x, tg, case, form, ticket)
        assert int(ticket) == 0, what
        again = _head_forward(hip, x, tg, case, form, ticket)
        assert int(ticket) == 0 and _same_bits(loss, again[0]) and _same_bits(sv, again[1]), what
        ref = H.head_ref(shape, regime, form, 0)
        worst['terms'] = max(worst.get('terms', 0), R.check(loss, ref['terms'], c['head.terms'], what + ' terms'))
        pick = sv['sem_pick'].cpu().long()
        assert torch.equal(pick, ref['sem_pick']), what + ' sem_pick'
        lab = case['tg']['mask_targets'].reshape(-1)
        if regime == 'ties' and C > 1:
            assert (pick == lab).any() and (pick != lab).any(), what
        if H.FORMS[form].get('unsup'):
            assert (loss[[0, 5, 6]] == 0).all(), what
        for gi, g in enumerate(H.G7):
            ref = H.head_ref(shape, regime, form, gi)
            d = hip.head_loss_backward(torch.tensor(g, device=hip_device), tg['mask_targets'], sv, K)
            for name in ('cls', 'bbox', 'surface', 'iou', 'iou_s', 'side'):
                worst[name] = max(worst.get(name, 0), R.check(d[name], ref['grads'][name], c['head.d_' + name],
                                                              f'{what} g{gi} d_{name}'))
            assert (d['bbox'][..., 3:] == 0).all(), what + ': size / yaw columns of d_bbox'
            side = d['side'].cpu()                                            # (6, B, C, 2K)
            written = torch.zeros(B * K, C, dtype=torch.bool)
            written.scatter_(1, pick[:, None], True).scatter_(1, lab[:, None], True)
            written = written.reshape(B, K, C).permute(0, 2, 1)               # (B, C, K)
            assert (side[..., K:] == 0).all() and (side[..., :K][:, ~written] == 0).all(), what + ' d_side'
            assert _same_bits(d, hip.head_loss_backward(torch.tensor(g, device=hip_device), tg['mask_targets'], sv, K))
    print(f'head loss {shape} {regime}: worst error / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))


def _saqe_forward(hip, xs, tg, pick, sup, ticket):
    return hip.saqe_extra_forward(xs['robj'], xs['rot'], xs['bbox'], xs['bbox_t'], xs['jsurf'], xs['side'], tg,
                                  pick, H.SAQE_CONFIG, sup, ticket)


@pytest.mark.parametrize('regime', H.REGIMES)
@pytest.mark.parametrize('shape', H.HEAD_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_saqe_extras_against_float64(hip_device, shape, regime):
    from nesie_amd.kernels import backend_for
    c = R.constants()
    B, K, Tn, C = shape
    case = H.head_case(shape, regime)
    xs, tg = _dev(case['saqe'], hip_device), _dev(case['tg'], hip_device)
    hip = backend_for(xs['rot'])
    ticket = _ticket(hip_device)
    pick64 = H.head_ref(shape, regime, 'sup0', 0)['sem_pick']
    pick = pick64.to(hip_device, torch.int32)
    lab = case['tg']['mask_targets'].reshape(-1)
    worst = {}
    for sup in (0, 1):
        what = f'{shape} {regime} sup {sup}'
        loss, sv = _saqe_forward(hip, xs, tg, pick, sup, ticket)
        assert int(ticket) == 0, what
        again = _saqe_forward(hip, xs, tg, pick, sup, ticket)
        assert int(ticket) == 0 and _same_bits(loss, again[0]) and _same_bits(sv, again[1]), what
        worst['terms'] = max(worst.get('terms', 0), R.check(loss, H.saqe_ref(shape, regime, sup, 0)['terms'],
                                                            c['saqe.terms'], what + ' terms'))
        if sup:
            assert float(loss[2]) == 0.0 and (sv['rot'] == 0).all(), what
        at_pick = torch.zeros(B * K, C, dtype=torch.bool).scatter_(1, pick64[:, None], True).reshape(B, K, C)
        at_pick = torch.cat([at_pick, at_pick], 1)                            # (B, 2K, C)
        assert (sv['rot'].cpu()[~at_pick] == 0).all(), what + ' s_rot'
        at_lab = torch.zeros(B * K, C, dtype=torch.bool).scatter_(1, lab[:, None], True)
        at_lab = at_lab.reshape(B, K, C).permute(0, 2, 1)                      # (B, C, K)
        for gi, g in enumerate(H.G4):
            ref = H.saqe_ref(shape, regime, sup, gi)
            d = hip.saqe_extra_backward(torch.tensor(g, device=hip_device), tg['mask_targets'], sv, K)
            for name in ('robj', 'angle', 'rot', 'side'):
                worst[name] = max(worst.get(name, 0), R.check(d[name], ref['grads'][name], c['saqe.d_' + name],
                                                              f'{what} g{gi} d_{name}'))
            side = d['side'].cpu()
            assert (side[..., :K] == 0).all() and (side[..., K:][:, ~at_lab] == 0).all(), what + ' d_side'
            assert (d['rot'].cpu()[~at_pick] == 0).all(), what + ' d_rot'
    print(f'saqe extras {shape} {regime}: worst error / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))


def _vote_forward(hip, v, ticket):
    return hip.vote_loss_forward(v['seed'], v['vote'], v['seed_idx'], v['mask'], v['targets'], H.VOTE_W, ticket)


@pytest.mark.parametrize('shape,regime,form,sup', [((8, 256, 64, 18), 'benign', 'sup2', 0),
                                                   ((8, 256, 64, 18), 'saturated', 'label', 1),
                                                   ((8, 256, 64, 18), 'ties', 'sup1', 1),
                                                   ((3, 70, 5, 18), 'weights', 'sup0', 0)])
def test_one_ticket_serves_the_three_kernels_back_to_back(hip_device, shape, regime, form, sup):
    """Head loss (32 workgroups at the training shape), SAQE extras (32) and vote loss (64) queued on
    one stream with one ticket, twice over, against the same calls on tickets of their own."""
    from nesie_amd.kernels import backend_for
    case = H.head_case(shape, regime)
    x, tg, xs = (_dev(case[k], hip_device) for k in ('x', 'tg', 'saqe'))
    v = _dev(H.vote_case(17000, 3, 'mixed'), hip_device)
    hip = backend_for(x['cls'])

    def run(tickets):
        out = []
        for _ in range(2):
            loss, sv = _head_forward(hip, x, tg, case, form, tickets[0])
            out += [loss, sv, _saqe_forward(hip, xs, tg, sv['sem_pick'], sup, tickets[1])[0]]
            out += list(_vote_forward(hip, v, tickets[2]))
        torch.cuda.synchronize(hip_device)
        return out
    shared = _ticket(hip_device)
    own = [_ticket(hip_device) for _ in range(3)]
    a, b = run([shared] * 3), run(own)
    assert int(shared) == 0 and all(int(t) == 0 for t in own)
    assert all(_same_bits(p, q) for p, q in zip(a, b))
    R.check(a[0], H.head_ref(shape, regime, form, 0)['terms'], R.constants()['head.terms'], 'terms')
    R.check(a[2], H.saqe_ref(shape, regime, sup, 0)['terms'], R.constants()['saqe.terms'], 'extras')


@pytest.mark.parametrize('shape', H.TARGET_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_head_targets_equal_the_tensor_ops(hip_device, shape):
    from nesie_amd.kernels import backend_for
    from nesie_amd.votenet import head_loss
    from nesie_amd.votenet.nesie_head import GTBatch, NesieHead
    c = _dev(H.target_case(shape), hip_device)
    got = backend_for(c['agg']).head_targets(c['agg'], c['gt_boxes'], c['gt_labels'], c['gt_count'],
                                             c['gt_valid'], H.POS_THR, H.NEG_THR)
    stub = types.SimpleNamespace(train_cfg=dict(pos_distance_thr=H.POS_THR, neg_distance_thr=H.NEG_THR))
    gt = GTBatch(c['gt_boxes'], c['gt_labels'], c['gt_count'], c['gt_valid'])
    head_loss.ENABLED = False
    try:
        want = NesieHead.get_targets(stub, c['agg'], gt, None, bbox_preds=dict(aggregated_points=c['agg']),
                                     vote_targets=(None, None))
    finally:
        head_loss.ENABLED = True
    names = (None, None, 'center_targets', 'bbox_targets', 'mask_targets', None, 'obj_targets', 'obj_weights',
             'box_weights', 'valid_weights', 'assignment')
    for name, w in zip(names, want):
        if name:
            assert got[name].dtype == w.dtype and got[name].shape == w.shape, name
            assert torch.equal(got[name], w), f'{shape} {name}'
    pos, some = got['obj_targets'] == 1, got['obj_weights'] > 0
    assert pos.any() and (some & ~pos).any() and (~some).any()       # positive, negative and ignored
    assert (c['gt_valid'].sum(1) == 0).any()                        # an empty scene


@pytest.mark.parametrize('gps', [1, 3])
@pytest.mark.parametrize('bn', list(H.VOTE_SIZES))
def test_vote_loss_against_float64(hip_device, bn, gps):
    from nesie_amd.kernels import backend_for
    c = R.constants()
    worst = 0.0
    for mask_kind in H.VOTE_MASKS:
        what = f'vote loss {bn} x {gps} {mask_kind}'
        v = _dev(H.vote_case(bn, gps, mask_kind), hip_device)
        hip = backend_for(v['vote'])
        ticket = _ticket(hip_device)
        loss, sign, scale = _vote_forward(hip, v, ticket)
        assert int(ticket) == 0, what
        again = _vote_forward(hip, v, ticket)
        assert int(ticket) == 0 and all(_same_bits(p, q) for p, q in zip((loss, sign, scale), again)), what
        ref = H.vote_ref(bn, gps, mask_kind)
        assert torch.equal(sign.cpu().double(), ref['sign']), what + ' sign'
        d_vote = hip.vote_loss_backward(torch.tensor(H.VOTE_G, device=hip_device), scale, sign)
        worst = max(worst, R.check(loss, ref['loss'], c['vote.loss'], what + ' loss'),
                    R.check(scale, ref['scale'], c['vote.scale'], what + ' scale'),
                    R.check(d_vote, ref['d_vote'], c['vote.d_vote'], what + ' d_vote'))
        if mask_kind == 'zeros':
            assert float(loss) == 0.0 and (sign == 0).all() and (d_vote == 0).all(), what
            torch.testing.assert_close(float(scale), H.VOTE_W / 1e-6, rtol=2.0 ** -22, atol=0)
    print(f'vote loss {bn} x {gps}: worst error / bound {worst:.3f}')


def _nan(*shape, device):
    return torch.full(shape, float('nan'), device=device)


@pytest.mark.parametrize('bins', H.DECODE_BINS)
@pytest.mark.parametrize('k', H.DECODE_K)
def test_side_decode_against_float64(hip_device, k, bins):
    from nesie_amd.kernels import backend_for
    c = R.constants()
    worst = {}
    for b, spread in itertools.product(H.DECODE_B, H.DECODE_SPREAD):
        case = _dev(H.decode_case(b, k, bins, spread), hip_device)
        hip = backend_for(case['reg'])
        probs, surface, bbox = (_nan(b, 6, bins, k, device=hip_device), _nan(b, k, 6, device=hip_device),
                                _nan(b, k, 7, device=hip_device))
        hip.side_decode_forward(case['reg'], case['agg'], case['scale'], case['sign'], probs, surface, bbox)
        for grads in H.DECODE_GRADS:
            what = f'decode B {b} K {k} bins {bins} spread {spread} d_{grads}'
            ref = H.decode_ref(b, k, bins, spread, grads)
            d_reg, d_agg = _nan(b, 6 * bins + 2, k, device=hip_device), _nan(b, k, 3, device=hip_device)
            hip.side_decode_backward(case['reg'], probs, case['scale'], case['sign'],
                                     case['d_surface'] if grads in ('surface', 'both') else None,
                                     case['d_bbox'] if grads in ('bbox', 'both') else None, d_reg, d_agg)
            for name, got in (('probs', probs), ('surface', surface), ('bbox', bbox), ('d_reg', d_reg), ('d_agg', d_agg)):
                worst[name] = max(worst.get(name, 0), R.check(got, ref[name], c['decode.' + name], f'{what} {name}'))
            if grads == 'surface':
                assert (d_reg[:, 6 * bins:] == 0).all(), what + ': heading gradient without d_bbox'
    print(f'side decode K {k} bins {bins}: worst error / bound ' + ', '.join(f'{n} {v:.3f}' for n, v in worst.items()))


@pytest.mark.parametrize('n', H.FINISH_N)
@pytest.mark.parametrize('ch', H.FINISH_C)
def test_vote_finish_against_float64(hip_device, ch, n):
    from nesie_amd.kernels import backend_for
    c = R.constants()
    case = _dev(H.finish_case(ch, n), hip_device)
    hip = backend_for(case['raw'])
    worst = {}
    for normalise in (True, False):
        points, feats, inv = hip.vote_finish_forward(case['raw'], case['seed_points'], case['seed_feats'], normalise)
        for grads in H.FINISH_GRADS:
            what = f'vote finish C {ch} n {n} normalise {normalise} d_{grads}'
            ref = H.finish_ref(ch, n, normalise, grads)
            d_raw = hip.vote_finish_backward(case['g_feats'] if grads in ('both', 'feats') else None,
                                             case['g_points'] if grads in ('both', 'points') else None,
                                             feats, inv, normalise)
            for name, got in (('points', points), ('feats', feats), ('inv_norm', inv), ('d_raw', d_raw)):
                worst[name] = max(worst.get(name, 0), R.check(got, ref[name], c['finish.' + name], f'{what} {name}'))
            if grads == 'feats':
                assert (d_raw[:, :3] == 0).all(), what
            if grads == 'points':
                assert (d_raw[:, 3:] == 0).all(), what
    print(f'vote finish C {ch} n {n}: worst error / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))

"""Shared by tests/test_emu_attn_shared.py and tests/test_gpu_attn_shared.py: the stand-alone checks of the shared-prompt decode attention
(csrc/rqt_attn_shared.hip) through rqamd_dbg_rqt_attn_shared.

The kernel's claim is exactness: output and appended key / value of row r are bit for bit those of rqamd_dbg_rqt_attn_decode on an expanded
cache [rows][nh][Ps + Tcap_row][64] that holds a copy of the group's prefix in front of the row's own positions.  Every case runs both
launches on the same inputs and compares bits; the group caches, every other own row and all guards must be untouched.  One case per form
is also held against the fp64 reference of tests/rqt_attn_cases.py within its C_BF16 bound.

Buffers are guarded and poisoned as in rqt_attn_cases.py: own rows >= t - Ps hold NaN, y starts as NaN.  No case reaches a kernel trap:
Ps <= t <= t_max < Ps + Tcap_row everywhere, and the refusals are host-side."""
import torch

import rqt_attn_cases as R

PS = (1, 3, 7, 8, 9, 31, 63)
FANS = (1, 2, 3, 5)
HEADS = (2, 5, 20)
TCAPS = (16, 64)


def t_values(Ps, Tcap):
    """Ps, Ps + 1, the next multiple of 8 minus 1, that multiple, Ps + Tcap - 1 (all inside the own cache by construction)"""
    m = (Ps // 8 + 1) * 8
    ts = [Ps, Ps + 1, m - 1, m, Ps + Tcap - 1]
    assert all(Ps <= t < Ps + Tcap for t in ts), (Ps, Tcap, ts)
    return sorted(set(ts))


def form(Ps, Tcap, t_max):
    """'small' (attn_shared_small_kernel: at most 8 keys) or 'reg' (attn_shared_kernel), the launcher's rule restated"""
    nj = min((t_max >> 3) + 1, (Ps + Tcap + 7) // 8)
    return 'small' if nj == 1 else 'reg'


class Case:
    pass


def make(G, fan, nh, Ps, Tcap, t, seed, dtype=torch.bfloat16, peaked=False):
    g = torch.Generator().manual_seed(seed)
    c = Case()
    rows = G * fan
    c.G, c.fan, c.rows, c.nh, c.Ps, c.Tcap, c.t, c.E, c.dtype = G, fan, rows, nh, Ps, Tcap, t, nh * 64, dtype
    q, c.k, c.v = (torch.randn((rows, nh, 64), generator=g).to(dtype) for _ in range(3))
    c.ks, c.vs = (torch.randn((G, nh, Ps, 64), generator=g).to(dtype) for _ in range(2))
    c.kc, c.vc = (torch.randn((rows, nh, Tcap, 64), generator=g).to(dtype) for _ in range(2))
    c.kc[:, :, t - Ps:] = float('nan')
    c.vc[:, :, t - Ps:] = float('nan')
    grp = torch.arange(rows) // fan
    c.kx = torch.cat([c.ks[grp], c.kc], dim=2).contiguous()             # the expanded caches of the plain kernel
    c.vx = torch.cat([c.vs[grp], c.vc], dim=2).contiguous()
    if peaked:                                                           # q = 8 x one key: a prefix key, an own key or this token's, by pair
        K = torch.cat([c.kx[:, :, :t], c.k[:, :, None]], dim=2).float()
        pair = torch.arange(rows * nh).view(rows, nh)
        win = torch.where(pair % 3 == 0, pair % Ps, torch.where(pair % 3 == 1, torch.full_like(pair, t), Ps + pair % max(t - Ps, 1)))
        win = win.clamp(max=t)
        q = (8.0 * torch.gather(K, 2, win[:, :, None, None].expand(rows, nh, 1, 64))[:, :, 0]).to(dtype)
    c.q = q
    c.qkv = torch.cat([q.reshape(rows, -1), c.k.reshape(rows, -1), c.v.reshape(rows, -1)], dim=-1).contiguous()
    return c


def run(nat, dev, c, t_max, step_base=None, half=False):
    """both launches -> (shared run, plain run on the expanded caches)"""
    kw = dict(half=True) if half else {}
    s, p = R.Run(), R.Run()
    for r in (s, p):
        r.qkv = R.Buf(c.qkv, dev)
        r.y = R.Buf(R.nan_like((c.rows, c.E), c.dtype), dev)
        r.step = R.Buf(torch.full((1,), -12345, dtype=torch.int32), dev) if step_base is not None else None
    s.ks, s.vs, s.kc, s.vc = (R.Buf(x, dev) for x in (c.ks, c.vs, c.kc, c.vc))
    p.kc, p.vc = R.Buf(c.kx, dev), R.Buf(c.vx, dev)
    nat.dbg_rqt_attn_shared(s.qkv.t, s.ks.t, s.vs.t, s.kc.t, s.vc.t, s.y.t, c.fan, c.nh, c.t, t_max=t_max,
                            step=s.step.t if s.step else None, step_base=step_base or 0, **kw)
    nat.dbg_rqt_attn_decode(p.qkv.t, p.kc.t, p.vc.t, p.y.t, c.nh, c.Ps + c.Tcap, c.t, t_max=t_max,
                            step=p.step.t if p.step else None, step_base=step_base or 0, **kw)
    return s, p


def verify(c, s, p, what, step_base=None):
    assert not bool(torch.isnan(p.y.t.float()).any()), f'{what}: the plain kernel read poison'
    assert R.same_bits(s.y.t, p.y.t), f'{what}: y differs from the plain kernel on the expanded cache'
    for name, own, exp, new, grp in (('K', s.kc, p.kc, c.k, s.ks), ('V', s.vc, p.vc, c.v, s.vs)):
        now = own.t.cpu()
        want = (c.kc if name == 'K' else c.vc).clone()
        want[:, :, c.t - c.Ps] = new
        assert R.same_bits(now, want), f'{what}: own {name} cache is not (old rows, this token at row {c.t - c.Ps}, poison beyond)'
        assert R.same_bits(now[:, :, c.t - c.Ps], exp.t.cpu()[:, :, c.t]), f'{what}: appended {name} row differs from the plain kernel\'s'
        assert R.same_bits(grp.t, c.ks if name == 'K' else c.vs), f'{what}: the group {name} cache changed'
        own.check_guard(f'{what} own {name} cache')
        grp.check_guard(f'{what} group {name} cache')
    s.y.check_guard(what + ' y')
    s.qkv.check_guard(what + ' qkv')
    assert R.same_bits(s.qkv.t, c.qkv), f'{what}: qkv changed'
    if s.step is not None:
        assert int(s.step.t.cpu()[0]) == step_base, f'{what}: the step counter changed'
        s.step.check_guard(what + ' step')


def exact_case(nat, dev, fan, nh, Ps, Tcap, t, step, half=False):
    G = 3 if fan == 1 else 2
    t_max = min(t | 7, Ps + Tcap - 1)                                   # the engine's bound: the last position of the 8-key bucket
    what = f'shared {form(Ps, Tcap, t_max)} G {G} fan {fan} nh {nh} Ps {Ps} Tcap_row {Tcap} t {t} t_max {t_max} step {step} half {half}'
    c = make(G, fan, nh, Ps, Tcap, t, seed=1 + 7 * t + 1009 * Tcap + 13 * fan + nh + 31 * Ps, dtype=torch.float16 if half else torch.bfloat16)
    step_base = t - min(t, 2) if step else None
    s, p = run(nat, dev, c, t_max, step_base, half)
    verify(c, s, p, what, step_base)


def exact_cases(nat, dev, Ps, half=False, thin=None):
    """every fan x nh x Tcap_row x t of the lists above at this Ps, t by value and through a device counter.  thin (an integer; the
    emulator, which runs a launch of 200 (row, head) pairs in a third of a second): every fan x nh x Tcap_row still, but one (t, counter
    form) each, rotating with `thin` so that the tests of a file cover every t in both forms at every Ps"""
    n = 0
    for fan in FANS:
        for nh in HEADS:
            for Tcap in TCAPS:
                ts = t_values(Ps, Tcap)
                pairs = [(t, step) for t in ts for step in (False, True)]
                if thin is not None:
                    pairs = [pairs[(n + thin) % len(pairs)]]
                for t, step in pairs:
                    exact_case(nat, dev, fan, nh, Ps, Tcap, t, step, half)
                n += 1
    return n


def fp64_case(nat, dev, which):
    """one case per form against the fp64 reference of rqt_attn_cases within C_BF16 (peaked queries: prefix keys, own keys and the token)"""
    fan, nh, Ps, Tcap, t = (3, 5, 3, 16, 6) if which == 'small' else (3, 5, 31, 64, 70)
    t_max = min(t | 7, Ps + Tcap - 1)
    assert form(Ps, Tcap, t_max) == which
    c = make(2, fan, nh, Ps, Tcap, t, seed=77, peaked=True)
    s, p = run(nat, dev, c, t_max)
    verify(c, s, p, f'shared {which} fp64')
    K = torch.cat([c.kx[:, :, :t].double(), c.k.double()[:, :, None]], dim=2).to(dev)
    V = torch.cat([c.vx[:, :, :t].double(), c.v.double()[:, :, None]], dim=2).to(dev)
    ref, A = R.attn_ref(c.q.double().to(dev)[:, :, None], K, V)
    return R.check(s.y.t.view(c.rows, nh, 1, 64), ref, A, 'bf16', 'shared-' + which, f'shared {which} vs fp64')


def refusals(nat, dev, pytest):
    """host refusals return the stated codes and leave y NaN"""
    def go(fan=2, nh=2, Ps=3, Tcap=16, t=5, t_max=7, drop=None, hd=64, rows=4):
        c = make(rows // fan if rows % fan == 0 else 2, fan, nh, Ps, Tcap, max(min(t, Ps + Tcap - 1), Ps), seed=5)
        b = {k: R.Buf(getattr(c, k), dev) for k in ('ks', 'vs', 'kc', 'vc')}
        if hd != 64:
            c.qkv, c.E = torch.zeros((c.rows, 3 * nh * hd), dtype=torch.bfloat16), nh * hd
        if rows % fan:
            c.qkv, c.rows = torch.zeros((rows, 3 * c.E), dtype=torch.bfloat16), rows
        qkv, y = R.Buf(c.qkv, dev), R.Buf(R.nan_like((c.rows, c.E)), dev)
        a = {k: (None if k == drop else v.t) for k, v in b.items()}
        try:
            nat.dbg_rqt_attn_shared(qkv.t, a['ks'], a['vs'], a['kc'], a['vc'], y.t, fan, nh, t, t_max=t_max)
        except Exception:
            assert bool(torch.isnan(y.t.float()).all()), 'a refused launch wrote y'
            y.check_guard('refused launch')
            raise
        assert not bool(torch.isnan(y.t.float()).any())
    go()                                                                   # (the arguments the refusals vary are valid ones)
    with pytest.raises(ValueError, match='inside the shared prefix'):
        go(t=2)
    with pytest.raises(ValueError, match='outside the own cache'):
        go(t=3 + 16, t_max=-1)
    for drop in ('ks', 'vs', 'kc', 'vc'):
        with pytest.raises(ValueError, match='null pointer'):
            go(drop=drop)
    with pytest.raises(ValueError, match='t_max'):
        go(t_max=19)
    with pytest.raises(ValueError, match='t 5 > t_max 4'):
        go(t_max=4)
    with pytest.raises(ValueError, match='in groups of 3'):
        go(fan=3, rows=4)
    with pytest.raises(NotImplementedError, match='head size 64 only'):
        go(hd=80)
    with pytest.raises(NotImplementedError, match='256 keys'):
        c = make(2, 2, 2, 63, 200, 70, seed=5)
        qkv, y = R.Buf(c.qkv, dev), R.Buf(R.nan_like((c.rows, c.E)), dev)
        try:
            nat.dbg_rqt_attn_shared(qkv.t, *(R.Buf(x, dev).t for x in (c.ks, c.vs, c.kc, c.vc)), y.t, 2, 2, 70, t_max=71)
        finally:
            assert bool(torch.isnan(y.t.float()).all())

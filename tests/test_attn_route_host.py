"""Which kernels the six ivh_flash_attn_* entry points launch (csrc/flash_attn.hip: one route function per direction, one launch table per kernel
file), seen through ivh_attn_debug_route: per launch {family, kind, HDP, flags, grid, block, dynamic LDS bytes, 0}.  Host logic only: the
"pointers" are numbers, nothing is launched and no device is touched.  A GPU test cannot tell which attention kernel ran -- the 16x16x32 and 32x32x16
families agree to tolerance, the packed and unpacked builds bit for bit -- so the shipped default is pinned here and nowhere else.

The route is held against `_model`, written from the launch rules and not from the C++:
  Refused, in this order: a null q / k / v; B, H, Lq or Lk <= 0; hd not a multiple of 8 in 8 .. 128; a q or k/v stride that is no multiple of 8; q, k or v
  not 16-byte aligned; B or H above 65535.  Forward then: out null, not 8-byte aligned or with a stride that is no multiple of 4.  Backward then: a null
  out / dq / dk / dv; an out stride that is no multiple of 8 or out not 16-byte aligned; a dq or dk/dv stride that is no multiple of 4.
  HDP = 64 / 96 / 128 for hd <= 64 / <= 96 / above.  Family 16 runs 64 rows per workgroup, family 32 runs 128 (256 as two wave groups, 512 threads);
  grid = ceil(L / rows) * H * B over Lq (forward, dQ) or Lk (dK/dV); 256 threads; no dynamic LDS but for the 32x32 dK/dV.
  Dropout entries: hd <= 64 or refused; the 16x16 <64, DROP> kernels whatever ivh_set_attn_kernel says.
  The 32x32 family takes a call whose nine q, k/v, out strides are multiples of 8, whose (Lk + 64) * sl, (Lq + 64) * qsl and (Lq + 64) * ol byte
  products stay below 2^31 - 2^20, and whose out (forward) or dq, dk, dv with all their strides multiples of 8 (backward) are 16-byte aligned.
  ivh_set_attn_kernel: 0 = 32x32 when it takes the call, 1 = never, 2 = 32x32 or refused.  A device-side clip count is refused unless 32x32 runs.
  Backward, 32x32: dQ, then dK/dV on 32x32 with 4 * 64 * HDP * 2 + ceil(Lq / 64) * 512 bytes of LDS when hd <= 96 and that is at most 80 KiB, else
  on the 16x16 kernel.  Both carry NP unless ivh_probe_attn32_unpacked(0) / IVH_ATTN_NOPK=0.
  Forward, 32x32, by ivh_probe_attn32_pingpong / IVH_ATTN_PP and the stamp buffer, `mid` = 64 < hd <= 96:
    modes 1 .. 5 run two wave groups when no stamp buffer is set or mid: with the buffer (at least 128 rows, or refused) STAMP, + NP from mode 4;
    without it mid modes 4 / 5 = NP / NP + PRIO, mid mode 3 = GSEL, anything else PRIO for mode 2 and plain otherwise.
    Everything else is the one-group kernel: mid without a buffer mode 7 = NP2 and mode 6 = NP; otherwise DEFER under IVH_ATTN_DEFER=1 (+ NP when
    unpacked and mid), else NP when unpacked, else plain -- and with a stamp buffer STAMP, refused when the grid exceeds the buffer's rows,
    under EVERY mode: that kernel stamps its whole grid."""
import ctypes as C
import itertools
import json
import os
import random
import subprocess
import sys

from internvideo_amd import lib

FWD, DQ, DKDV, FWD2 = range(4)
DROP, DEFER, NP, NP2, PRIO, GSEL, STAMP = (1 << i for i in range(7))
ADDR = ("q", "k", "v", "out", "dq", "dk", "dv")
STRIDES = ("q", "kv", "o", "dq", "dkv")
LIM = 2 ** 31 - 2 ** 20
BASE = 0x10000000
ENV = ("IVH_ATTN_PP", "IVH_ATTN_NOPK", "IVH_ATTN_DEFER")


def packed(B, L, H, hd, **kw):
    """q, k, v thirds of one [B * L, 3 * D] buffer, gradients likewise, out [B * L, D]"""
    D = H * hd
    s3, s1 = (L * 3 * D, 3 * D, hd), (L * D, D, hd)
    addr = dict(q=BASE, k=BASE + 2 * D, v=BASE + 4 * D, out=2 * BASE, dq=3 * BASE, dk=3 * BASE + 2 * D, dv=3 * BASE + 4 * D)
    return dict(dict(bwd=0, dropout=0, nb=0, B=B, H=H, Lq=L, Lk=L, hd=hd, addr=addr, strides=dict(q=s3, kv=s3, o=s1, dq=s3, dkv=s3)), **kw)


def separate(B, Lq, Lk, H, hd, **kw):
    """contiguous q [B, Lq, H, hd] and k, v [B, Lk, H, hd]; out and dq like q, dk and dv like k"""
    sq, sk = (Lq * H * hd, H * hd, hd), (Lk * H * hd, H * hd, hd)
    addr = {n: (i + 1) * BASE for i, n in enumerate(ADDR)}
    return dict(dict(bwd=0, dropout=0, nb=0, B=B, H=H, Lq=Lq, Lk=Lk, hd=hd, addr=addr, strides=dict(q=sq, kv=sk, o=sq, dq=sq, dkv=sk)), **kw)


def _with(case, addr=None, strides=None, **kw):
    return dict(case, addr=dict(case["addr"], **(addr or {})), strides=dict(case["strides"], **(strides or {})), **kw)


def _flat(c):
    return [c["bwd"], c["dropout"], [c["addr"][n] for n in ADDR], [s for n in STRIDES for s in c["strides"][n]], c["B"], c["H"], c["Lq"], c["Lk"], c["hd"], c["nb"]]


def _call(L, flat):
    """-> the launches as 8-tuples, or the refusal's message"""
    bwd, dropout, addr, strides, *dims = flat
    out = (C.c_int32 * 16)(*([-1] * 16))
    n = L.ivh_attn_debug_route(bwd, dropout, (C.c_uint64 * 7)(*addr), (C.c_int64 * 15)(*strides), *dims, out)
    assert n == (0 if n == 0 else 2 if bwd else 1), n
    assert list(out)[8 * n:] == [-1] * (16 - 8 * n)
    return [tuple(out[8 * i:8 * i + 8]) for i in range(n)] if n else L.ivh_last_error().decode()


def _route(L, case):
    return _call(L, _flat(case))


def _model(c, choice=0, pp=0, unpacked=1, defer=0, stamp_rows=None):
    """the rules of the module docstring -> the launches, or the text a refusal must carry.  stamp_rows: rows of the stamp buffer, None = not set"""
    a, s, B, H, Lq, Lk, hd = c["addr"], c["strides"], c["B"], c["H"], c["Lq"], c["Lk"], c["hd"]
    mult = lambda names, m: all(x % m == 0 for n in names for x in s[n])
    name = "flash_attn_%s%s" % ("bwd" if c["bwd"] else "fwd", "_dropout" if c["dropout"] else "")
    if not (a["q"] and a["k"] and a["v"]):
        return "flash_attn: null q/k/v"
    if min(B, H, Lq, Lk) <= 0:
        return f"flash_attn: empty problem B={B} H={H} Lq={Lq} Lk={Lk}"
    if hd <= 0 or hd % 8 or hd > 128:
        return f"flash_attn: head dim {hd} not supported (multiple of 8, <= 128)"
    if not mult(("q", "kv"), 8):
        return "flash_attn: strides must be multiples of 8 elements"
    if a["q"] % 16 or a["k"] % 16 or a["v"] % 16:
        return "flash_attn: q/k/v must be 16-byte aligned"
    if H > 65535 or B > 65535:
        return "flash_attn: B, H must be <= 65535"
    if not c["bwd"] and (not a["out"] or a["out"] % 8 or not mult(("o",), 4)):
        return f"{name}: bad out"
    if c["bwd"]:
        if not (a["out"] and a["dq"] and a["dk"] and a["dv"]):
            return f"{name}: null argument"
        if not mult(("o",), 8) or a["out"] % 16:
            return f"{name}: out/dout alignment"
        if not mult(("dq", "dkv"), 4):
            return f"{name}: dq/dk/dv strides must be multiples of 4"
    hdp = 64 if hd <= 64 else 96 if hd <= 96 else 128
    grid = lambda L_, rows: -(-L_ // rows) * H * B
    launch = lambda fam, kind, flags, L_, rows, block=256, lds=0: (fam, kind, hdp, flags, grid(L_, rows), block, lds, 0)
    small = lambda flags: [launch(16, DQ, flags, Lq, 64), launch(16, DKDV, flags, Lk, 64)] if c["bwd"] else [launch(16, FWD, flags, Lq, 64)]
    if c["dropout"]:
        return small(DROP) if hd <= 64 else f"{name}: built for head dims <= 64 (got {hd})"
    fits = mult(("q", "kv", "o"), 8) and (Lk + 64) * s["kv"][1] * 2 < LIM and (Lq + 64) * s["q"][1] * 2 < LIM and (Lq + 64) * s["o"][1] * 2 < LIM
    if c["bwd"]:
        ok32 = fits and mult(("dq", "dkv"), 8) and not (a["dq"] % 16 or a["dk"] % 16 or a["dv"] % 16)
    else:
        ok32 = fits and a["out"] % 16 == 0
    if choice == 2 and not ok32:
        return ("flash_attn_bwd: the 32x32 kernels were requested but do not support these strides / sizes" if c["bwd"] else
                "flash_attn_fwd: the 32x32 kernel was requested but does not support these strides / sizes")
    use32 = ok32 and choice != 1
    if c["nb"] and not use32:
        return ("flash_attn_bwd_dyn: a device-side clip count needs the 32x32 dQ kernel, which does not support this layout" if c["bwd"] else
                "flash_attn_fwd_dyn: a device-side clip count needs the 32x32 kernels, which do not support this layout")
    if not use32:
        return small(0)
    np_ = NP if unpacked else 0
    if c["bwd"]:
        lds = 4 * 64 * hdp * 2 + -(-Lq // 64) * 512
        big = hd <= 96 and lds <= 80 * 1024
        return [launch(32, DQ, np_, Lq, 128), launch(32, DKDV, np_, Lk, 128, lds=lds) if big else launch(16, DKDV, 0, Lk, 64)]
    mid, stamps = hdp == 96, stamp_rows is not None
    if 1 <= pp <= 5 and (mid or not stamps):
        if stamps:
            if stamp_rows < 128:
                return "flash_attn_fwd: the two-group stamp buffer holds 2 x 256 uint64"
            flags = STAMP | (NP if pp >= 4 else 0)
        elif mid and pp >= 3:
            flags = {3: GSEL, 4: NP, 5: NP | PRIO}[pp]
        else:
            flags = PRIO if pp == 2 else 0
        return [launch(32, FWD2, flags, Lq, 256, block=512)]
    if mid and not stamps and pp in (6, 7):
        return [launch(32, FWD, NP if pp == 6 else NP2, Lq, 128)]
    flags = (DEFER | (np_ if mid else 0)) if defer else np_
    if stamps and grid(Lq, 128) > stamp_rows:
        return f"flash_attn_fwd: the stamp buffer holds {stamp_rows} workgroups"
    return [launch(32, FWD, flags | (STAMP if stamps else 0), Lq, 128)]


def _grid():
    """the case grid: head dims x layouts (Lq != Lk, Lq = 1) x directions x plain / nb_dev / dropout, then one defect at a time on the 1B-like shape"""
    cases = []
    for hd, nb, bwd in itertools.product((64, 88, 96, 104, 128, 84, 136), (0, 1), (0, 1)):
        shapes = [packed(2, 417, 4, hd), separate(2, 417, 417, 4, hd), separate(3, 1, 77, 2, hd), separate(1, 130, 64, 3, hd), separate(2, 4097, 50, 1, hd),
                  separate(1, 6145, 6145, 1, hd)]
        cases += [dict(c, bwd=bwd, nb=nb) for c in shapes]
        if not nb:
            cases += [dict(c, bwd=bwd, dropout=1) for c in shapes[:3]]
    for hd, nb, bwd in itertools.product((64, 88, 128), (0, 1), (0, 1)):
        defects = []
        for base in (packed(2, 417, 4, hd, bwd=bwd, nb=nb), separate(2, 417, 100, 4, hd, bwd=bwd, nb=nb)):
            for n in ("o", "dq", "dkv"):                                      # a stride that is a multiple of 4 and not of 8, and one of 2
                b_, l_, h_ = base["strides"][n]
                defects += [_with(base, strides={n: (b_, l_ + 4, h_)}), _with(base, strides={n: (b_ + 4, l_, h_)}), _with(base, strides={n: (b_, l_, h_ + 2)})]
            for n in ("out", "dq", "dk", "dv"):                               # 8- but not 16-byte aligned; 4-byte aligned
                defects += [_with(base, addr={n: base["addr"][n] + 8}), _with(base, addr={n: base["addr"][n] + 4}), _with(base, addr={n: 0})]
            for n in ("q", "k", "v"):
                defects += [_with(base, addr={n: base["addr"][n] + 8}), _with(base, addr={n: 0})]
            for n in ("q", "kv", "o"):                                        # a slice past the 31-bit limit, and the last one below it
                b_, l_, h_ = base["strides"][n]
                L_ = base["Lk"] if n == "kv" else base["Lq"]
                edge = -(-LIM // (2 * (L_ + 64)) // 8) * 8
                defects += [_with(base, strides={n: (b_, 1 << 22, h_)}), _with(base, strides={n: (b_, edge, h_)}), _with(base, strides={n: (b_, edge - 8, h_)})]
            defects += [_with(base, strides={"q": (base["strides"]["q"][0], base["strides"]["q"][1] + 4, hd)}), dict(base, B=0), dict(base, Lk=0), dict(base, H=65536),
                      dict(base, B=65536)]
        cases += defects + [dict(c, dropout=1) for c in defects if not nb]          # the dropout entries make the same checks under their own names
    return cases


class _Switches:
    """process-wide switches for a block of parent-process checks; back to the defaults (automatic, one group, unpacked) on the way out"""
    def __init__(self, L, choice=0, pp=0, unpacked=1):
        self.L, self.v = L, (choice, pp, unpacked)

    def __enter__(self):
        for fn, v in zip(("ivh_set_attn_kernel", "ivh_probe_attn32_pingpong", "ivh_probe_attn32_unpacked"), self.v):
            assert getattr(self.L, fn)(v) == 0

    def __exit__(self, *exc):
        for fn, v in zip(("ivh_set_attn_kernel", "ivh_probe_attn32_pingpong", "ivh_probe_attn32_unpacked"), (0, 0, 1)):
            assert getattr(self.L, fn)(v) == 0


def test_route_follows_the_launch_rules_on_the_whole_grid():
    L = lib.load()
    cases, seen = _grid(), dict(refused=set(), keys=set())
    for choice in (0, 1, 2):
        with _Switches(L, choice=choice):
            for c in cases:
                got, want = _route(L, c), _model(c, choice=choice)
                assert got == want, (choice, c, got, want)
                if isinstance(got, str):
                    seen["refused"].add(got.split("B=")[0].split(" dim ")[0].split("(got")[0])
                else:
                    seen["keys"].update(r[:4] for r in got)
    assert len(seen["refused"]) == 20, sorted(seen["refused"])               # every refusal a route can make without a stamp buffer
    hdps = (64, 96, 128)
    assert seen["keys"] == ({(16, k, h, 0) for k in (FWD, DQ, DKDV) for h in hdps} | {(16, k, 64, DROP) for k in (FWD, DQ, DKDV)} |
                            {(32, k, h, NP) for k in (FWD, DQ) for h in hdps} | {(32, DKDV, 64, NP), (32, DKDV, 96, NP)}), sorted(seen["keys"])
    rng = random.Random(7)                                                   # a sweep over what the grid holds fixed
    with _Switches(L):
        for _ in range(3000):
            hd = rng.choice((8, 24, 64, 72, 88, 96, 104, 128, 20, 160))
            B, H, Lq, Lk = rng.choice((1, 3, 128)), rng.choice((1, 5, 16)), rng.choice((1, 63, 64, 417, 833, 4096, 4097, 6144, 6145, 9000)), rng.choice((1, 65, 417, 833))
            c = packed(B, Lq, H, hd) if rng.random() < 0.4 else separate(B, Lq, Lk, H, hd)
            c = dict(c, bwd=rng.randrange(2), nb=rng.randrange(2), dropout=int(rng.random() < 0.2))
            c = dict(c, nb=0) if c["dropout"] else c
            if rng.random() < 0.5:
                n = rng.choice(STRIDES)
                st = list(c["strides"][n])
                st[rng.randrange(3)] += rng.choice((2, 4, 8, 1 << 21, 1 << 24))
                c = _with(c, strides={n: tuple(st)})
            if rng.random() < 0.3:
                n = rng.choice(ADDR)
                c = _with(c, addr={n: c["addr"][n] + rng.choice((4, 8, 16))})
            assert _route(L, c) == _model(c), c


def test_probe_modes_and_unpacked_switch_without_a_stamp_buffer():
    L = lib.load()
    shapes = [packed(2, 417, 4, hd, nb=nb) for hd in (64, 88, 96, 104, 128) for nb in (0, 1)] + [separate(1, 300, 77, 2, 72), separate(1, 1, 9, 1, 40)]
    keys = set()
    for pp, unpacked in itertools.product(range(8), (0, 1)):
        with _Switches(L, pp=pp, unpacked=unpacked):
            for c, bwd in itertools.product(shapes, (0, 1)):
                got = _route(L, dict(c, bwd=bwd))
                assert got == _model(dict(c, bwd=bwd), pp=pp, unpacked=unpacked), (pp, unpacked, c, got)
                keys.update(r[:4] for r in got)
            # modes 3 / 4 / 5 outside 64 < hd <= 96 run as mode 1; the 16x16 kernels and the dropout entries do not look at the switches
            for hd in (64, 128):
                assert _route(L, packed(2, 417, 4, hd))[0][:4] == ((32, FWD2, hd, PRIO if pp == 2 else 0) if 1 <= pp <= 5 else (32, FWD, hd, NP * unpacked))
            assert _route(L, packed(2, 77, 4, 64, dropout=1)) == [(16, FWD, 64, DROP, 16, 256, 0, 0)]
    assert {k for k in keys if k[1] in (FWD, FWD2) and k[2] == 96} == {(32, FWD, 96, f) for f in (0, NP, NP2)} | {(32, FWD2, 96, f) for f in (0, PRIO, GSEL, NP, NP | PRIO)}
    assert L.ivh_probe_attn32_pingpong(8) != 0 and L.ivh_last_error().decode().startswith("ivh_probe_attn32_pingpong: 0 (off), 1 (two wave groups)")
    assert L.ivh_set_attn_kernel(3) != 0 and L.ivh_last_error().decode() == "ivh_set_attn_kernel: choice must be 0 (auto), 1 (16x16x32) or 2 (32x32x16)"


def test_pinned_rows_of_the_headline_steps():
    L = lib.load()
    with _Switches(L):
        for nb in (0, 1):                                                    # the 1B step, with and without DropPath sample skipping
            step = packed(128, 417, 16, 88, nb=nb)
            assert _route(L, step) == [(32, FWD, 96, NP, 8192, 256, 0, 0)]
            assert _route(L, dict(step, bwd=1)) == [(32, DQ, 96, NP, 8192, 256, 0, 0), (32, DKDV, 96, NP, 8192, 256, 52736, 0)]
        big = packed(32, 833, 25, 128, bwd=1)                                # the 6B shape: dK/dV stays on the 16x16 kernel above hd 96
        assert _route(L, big) == [(32, DQ, 128, NP, 7 * 25 * 32, 256, 0, 0), (16, DKDV, 128, 0, 14 * 25 * 32, 256, 0, 0)]
        assert _route(L, dict(big, nb=1)) == _route(L, big)
        assert _route(L, dict(big, bwd=0)) == [(32, FWD, 128, NP, 7 * 25 * 32, 256, 0, 0)]
        text = separate(16, 32, 32, 12, 64, dropout=1)                       # the text tower: dropout on the probabilities
        assert _route(L, text) == [(16, FWD, 64, DROP, 192, 256, 0, 0)]
        assert _route(L, dict(text, bwd=1)) == [(16, DQ, 64, DROP, 192, 256, 0, 0), (16, DKDV, 64, DROP, 192, 256, 0, 0)]
        assert _route(L, packed(2, 417, 16, 88, dropout=1)) == "flash_attn_fwd_dropout: built for head dims <= 64 (got 88)"
        assert _route(L, packed(2, 417, 16, 88, dropout=1, bwd=1)) == "flash_attn_bwd_dropout: built for head dims <= 64 (got 88)"
        # the LDS rule of the 32x32 dK/dV kernel: 80 KiB hold 4096 queries at HDP 96 and 6144 at HDP 64
        for hd, Lq in ((88, 4096), (64, 6144)):
            assert _route(L, separate(1, Lq, 64, 2, hd, bwd=1))[1][:7] == (32, DKDV, 64 if hd == 64 else 96, NP, 2, 256, 80 * 1024)
            assert _route(L, separate(1, Lq + 1, 64, 2, hd, bwd=1))[1] == (16, DKDV, 64 if hd == 64 else 96, 0, 2, 256, 0, 0)


def test_refusals_carry_the_entry_points_own_messages():
    L = lib.load()
    p, s = packed(2, 417, 4, 88), separate(2, 417, 100, 4, 88)
    odd_o = dict(o=(417 * 352, 356, 88))
    cases = (
        (0, _with(p, addr=dict(k=0)), "flash_attn: null q/k/v"),
        (0, dict(p, Lq=0), "flash_attn: empty problem B=2 H=4 Lq=0 Lk=417"),
        (0, packed(2, 417, 4, 84), "flash_attn: head dim 84 not supported (multiple of 8, <= 128)"),
        (0, dict(packed(2, 417, 4, 136), bwd=1), "flash_attn: head dim 136 not supported (multiple of 8, <= 128)"),
        (0, _with(s, strides=dict(kv=(100 * 352, 356, 88))), "flash_attn: strides must be multiples of 8 elements"),
        (0, _with(p, addr=dict(v=p["addr"]["v"] + 8)), "flash_attn: q/k/v must be 16-byte aligned"),
        (0, dict(p, H=65536), "flash_attn: B, H must be <= 65535"),
        (0, _with(p, addr=dict(out=0)), "flash_attn_fwd: bad out"),
        (0, _with(p, addr=dict(out=p["addr"]["out"] + 4)), "flash_attn_fwd: bad out"),
        (0, _with(p, strides=dict(o=(417 * 352, 354, 88))), "flash_attn_fwd: bad out"),
        (0, _with(packed(2, 9, 4, 64, dropout=1), addr=dict(out=0)), "flash_attn_fwd_dropout: bad out"),
        (2, _with(p, strides=odd_o), "flash_attn_fwd: the 32x32 kernel was requested but does not support these strides / sizes"),
        (2, _with(p, addr=dict(out=p["addr"]["out"] + 8)), "flash_attn_fwd: the 32x32 kernel was requested but does not support these strides / sizes"),
        (0, _with(p, strides=odd_o, nb=1), "flash_attn_fwd_dyn: a device-side clip count needs the 32x32 kernels, which do not support this layout"),
        (1, dict(p, nb=1), "flash_attn_fwd_dyn: a device-side clip count needs the 32x32 kernels, which do not support this layout"),
        (0, _with(p, bwd=1, addr=dict(dk=0)), "flash_attn_bwd: null argument"),
        (0, _with(p, bwd=1, strides=odd_o), "flash_attn_bwd: out/dout alignment"),
        (0, _with(p, bwd=1, addr=dict(out=p["addr"]["out"] + 8)), "flash_attn_bwd: out/dout alignment"),
        (0, _with(p, bwd=1, strides=dict(dq=(417 * 1056, 1058, 88))), "flash_attn_bwd: dq/dk/dv strides must be multiples of 4"),
        (0, _with(packed(2, 9, 4, 64, dropout=1, bwd=1), addr=dict(dv=0)), "flash_attn_bwd_dropout: null argument"),
        (0, _with(packed(2, 9, 4, 64, dropout=1, bwd=1), addr=dict(out=8)), "flash_attn_bwd_dropout: out/dout alignment"),
        (0, _with(packed(2, 9, 4, 64, dropout=1, bwd=1), strides=dict(dkv=(9 * 768, 770, 64))), "flash_attn_bwd_dropout: dq/dk/dv strides must be multiples of 4"),
        (2, _with(p, bwd=1, strides=dict(dkv=(417 * 1056, 1060, 88))), "flash_attn_bwd: the 32x32 kernels were requested but do not support these strides / sizes"),
        (2, _with(p, bwd=1, strides=dict(q=(417 * 1056, 1 << 22, 88))), "flash_attn_bwd: the 32x32 kernels were requested but do not support these strides / sizes"),
        (0, _with(p, bwd=1, nb=1, addr=dict(dq=p["addr"]["dq"] + 8)), "flash_attn_bwd_dyn: a device-side clip count needs the 32x32 dQ kernel, which does not support this layout"),
        (1, dict(p, bwd=1, nb=1), "flash_attn_bwd_dyn: a device-side clip count needs the 32x32 dQ kernel, which does not support this layout"),
    )
    for choice, c, text in cases:
        with _Switches(L, choice=choice):
            assert _route(L, c) == text, (choice, c)
        assert _model(c, choice=choice) == text
    # what choice 2 / a clip count refuse, choice 0 runs on the 16x16 kernels; a dK/dV that stays there does not stop a clip count
    with _Switches(L):
        assert _route(L, _with(p, strides=odd_o)) == [(16, FWD, 96, 0, 7 * 8, 256, 0, 0)]
        assert [r[:3] for r in _route(L, _with(p, bwd=1, addr=dict(dv=p["addr"]["dv"] + 8)))] == [(16, DQ, 96), (16, DKDV, 96)]
        assert [r[:2] for r in _route(L, packed(2, 417, 4, 128, bwd=1, nb=1))] == [(32, DQ), (16, DKDV)]


_CHILD = """
import ctypes as C, json, sys
L = C.CDLL(sys.argv[1])
L.ivh_last_error.restype = C.c_char_p
L.ivh_attn32_debug_stamps.argtypes = [C.c_void_p, C.c_int64]
setup, queries = json.loads(sys.stdin.read())
if setup["stamp_rows"] is not None:          # an address that is never dereferenced: this process only asks for routes
    L.ivh_attn32_debug_stamps(0x7f0000000000, setup["stamp_rows"])
if setup["pp"] is not None:
    assert L.ivh_probe_attn32_pingpong(setup["pp"]) == 0
res = []
for bwd, dropout, addr, strides, *dims in queries:
    out = (C.c_int32 * 16)(*([-1] * 16))
    n = L.ivh_attn_debug_route(bwd, dropout, (C.c_uint64 * 7)(*addr), (C.c_int64 * 15)(*strides), *dims, out)
    res.append([list(out[8 * i:8 * i + 8]) for i in range(n)] if n else L.ivh_last_error().decode())
print(json.dumps(res))
"""


def _child_routes(cases, env=None, pp=None, stamp_rows=None):
    """the routes of `cases` in a fresh process that loads the library alone and launches nothing (the IVH_ATTN_* variables are read once per process; a
    stamp buffer must never be left set in a process that runs kernels)"""
    keep = {k: v for k, v in os.environ.items() if k not in ENV}
    r = subprocess.run([sys.executable, "-c", _CHILD, lib.LIB_PATH], input=json.dumps([dict(pp=pp, stamp_rows=stamp_rows), [_flat(c) for c in cases]]),
                       capture_output=True, text=True, timeout=120, env=dict(keep, **(env or {})))
    assert r.returncode == 0, r.stderr
    return [[tuple(x) for x in v] if isinstance(v, list) else v for v in json.loads(r.stdout)]


def test_environment_switches_show_in_the_route():
    cases = [packed(2, 417, 4, hd, bwd=bwd) for hd in (64, 88, 128) for bwd in (0, 1)]
    for env, kw in ((dict(IVH_ATTN_NOPK="0"), dict(unpacked=0)), (dict(IVH_ATTN_NOPK="1"), {}), (dict(IVH_ATTN_DEFER="1"), dict(defer=1)),
                    (dict(IVH_ATTN_DEFER="1", IVH_ATTN_NOPK="0"), dict(defer=1, unpacked=0)), (dict(IVH_ATTN_DEFER="0"), {}), (dict(IVH_ATTN_PP="4"), dict(pp=4)),
                    (dict(IVH_ATTN_PP="6", IVH_ATTN_NOPK="0"), dict(pp=6, unpacked=0)), (dict(IVH_ATTN_PP="2", IVH_ATTN_DEFER="1"), dict(pp=2, defer=1)),
                    (dict(IVH_ATTN_PP="9"), dict(pp=9))):
        got = _child_routes(cases, env=env)
        assert got == [_model(c, **kw) for c in cases], (env, got)
    fwd = lambda env: [r[0][:4] for r in _child_routes(cases[::2], env=env)]
    assert fwd(dict(IVH_ATTN_DEFER="1")) == [(32, FWD, 64, DEFER), (32, FWD, 96, DEFER | NP), (32, FWD, 128, DEFER)]
    assert fwd(dict(IVH_ATTN_NOPK="0")) == [(32, FWD, 64, 0), (32, FWD, 96, 0), (32, FWD, 128, 0)]
    assert fwd(dict(IVH_ATTN_PP="6", IVH_ATTN_NOPK="0")) == [(32, FWD, 64, 0), (32, FWD, 96, NP), (32, FWD, 128, 0)]


def test_stamp_buffer_capacity_belongs_to_the_routed_kernel():
    small, large = packed(2, 417, 4, 64), packed(128, 417, 16, 64)           # 32 and 8192 one-group workgroups
    refusal = "flash_attn_fwd: the stamp buffer holds 128 workgroups"
    # mode 1, hd 64, a buffer sized for the two-group probe: the one-group kernel runs and stamps its whole grid, so the grid must fit
    assert _child_routes([large, small, dict(large, bwd=1)], pp=1, stamp_rows=128) == [refusal, [(32, FWD, 64, NP | STAMP, 32, 256, 0, 0)],
                                                                                      [(32, DQ, 64, NP, 8192, 256, 0, 0), (32, DKDV, 64, NP, 8192, 256, 36352, 0)]]
    cases = [packed(B, 417, H, hd, nb=nb) for B, H in ((2, 4), (128, 16)) for hd in (64, 88, 128) for nb in (0, 1)] + [separate(1, 129, 50, 64, 96), separate(1, 128, 50, 64, 96)]
    for pp, rows in itertools.product(range(8), (64, 128, 1 << 20)):
        got = _child_routes(cases, pp=pp, stamp_rows=rows)
        assert got == [_model(c, pp=pp, stamp_rows=rows) for c in cases], (pp, rows, got)
        for c, r in zip(cases, got):
            if isinstance(r, str):
                continue
            two = 1 <= pp <= 5 and 64 < c["hd"] <= 96
            assert r[0][1] == (FWD2 if two else FWD) and r[0][3] & STAMP and (two or r[0][4] <= rows), (pp, rows, c, r)
        assert any(isinstance(r, str) for r in got) == (rows < (1 << 20))
    assert _child_routes([packed(2, 417, 4, 88)], pp=5, stamp_rows=127) == ["flash_attn_fwd: the two-group stamp buffer holds 2 x 256 uint64"]
    assert _child_routes([packed(2, 417, 4, 88)], pp=5, stamp_rows=128) == [[(32, FWD2, 96, NP | STAMP, 16, 512, 0, 0)]]
    assert _child_routes([large, small], env=dict(IVH_ATTN_PP="3"), stamp_rows=128) == [refusal, [(32, FWD, 64, NP | STAMP, 32, 256, 0, 0)]]
    assert _child_routes([large, small], stamp_rows=128) == [refusal, [(32, FWD, 64, NP | STAMP, 32, 256, 0, 0)]]      # mode 0: refused before, too


def test_composed_signatures_equal_the_hand_written_lists():
    _vp, _i32, _i64, _f32, _u32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_uint32
    literal = {
        "ivh_flash_attn_fwd_dyn": [_vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp,
                                   _i32, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _vp],
        "ivh_flash_attn_bwd_dyn": [_vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _vp, _vp,
                                   _vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _vp],
        "ivh_flash_attn_fwd": [_vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp,
                               _i32, _i32, _i32, _i32, _i32, _f32, _vp, _vp],
        "ivh_flash_attn_bwd": [_vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _vp, _vp,
                               _vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _f32, _vp, _vp],
        "ivh_flash_attn_fwd_dropout": [_vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp,
                                       _i32, _i32, _i32, _i32, _i32, _f32, _vp, _f32, _u32, _vp],
        "ivh_flash_attn_bwd_dropout": [_vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _vp, _vp,
                                       _vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _f32, _vp, _f32, _u32, _vp],
        "ivh_probe_attn32_fwd_qkn": [_vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp,
                                     _i32, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _vp],
    }
    for name, argtypes in literal.items():
        assert lib.SIGNATURES[name] == argtypes, name
        assert list(getattr(lib.load(), name).argtypes) == argtypes, name

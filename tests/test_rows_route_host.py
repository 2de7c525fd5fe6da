"""Which kernel the six ivh_rmsnorm_add_* entry points launch (csrc/norms.hip: one route function and one launcher per direction, the width map
of csrc/common.h), seen through ivh_rmsnorm_add_debug_route: {b16, nch_t, wpr, rows, extra, skip, res_bf16, grid, shmem_bytes}.  Host logic only;
the "pointers" are bits of a mask, nothing is launched and no device is touched.  A GPU test cannot tell rmsnorm_add_bwd_b16_kernel (174 us per
launch at M = 53376, D = 1408) from the generic backward (247 us): they give the same numbers.  This can.

The route is held against `_model`, written from the launch rules and not from the C++:
  nch = ceil(D / 8 / 64), n4 = ceil(D / 8 / 256); grid = clamp(ceil(M / 4), 1, 8192) forward, clamp(ceil(M / 4), 1, cap) backward with cap = 512
  unless IVH_BWD_PARTS (64 .. 8192) says otherwise; the generic backward takes 16 * D bytes of LDS, everything else none.
  skip = the _skip entry (with or without maps); res_bf16 = 0 plain, 1 _bf16res, the flag on _skip.
  b16 (backward, bf16 stream): dy, dres_out, res_out, branch, gamma, dres_in, dbranch, dw_part, dgamma_part, dbias_part all set, nch <= 8,
  IVH_BWD_ROWS != 0, M * D * 2 < 2^31.  Then nch_t = n4, extra = dres_extra set, rows = 1 with extra or on _skip, else by IVH_BWD_ROWS (default 1):
  4 / 2 / 1 at n4 = 1, 2 / 1 at n4 = 2.  Everything else is generic: nch 1 .. 4 -> <nch, 1>, 5 .. 8 -> <2, 4>, wider rows are refused.
  Fields that do not apply (wpr of the b16 kernel, rows of the generic ones) read 0."""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys

from internvideo_amd import lib

FIELDS = ("b16", "nch_t", "wpr", "rows", "extra", "skip", "res_bf16", "grid", "shmem_bytes")
FWD_ARGS = ("res_in", "branch", "gamma", "rowscale", "w", "res_out", "y", "rstd", "branch_slot", "y_slot")
BWD_ARGS = ("dy", "dres_out", "res_out", "rstd", "w", "branch", "gamma", "rowscale", "dres_in", "dbranch", "dw_part", "dgamma_part", "dbias_part",
            "dres_extra", "y_slot", "branch_slot")
INTERIOR = ("dy", "dres_out", "res_out", "branch", "gamma", "dres_in", "dbranch", "dw_part", "dgamma_part", "dbias_part")
PLAIN, BF16RES, SKIP_F32, SKIP_BF16 = range(4)
ENTRY = ("rmsnorm_add_%s", "rmsnorm_add_%s_bf16res", "rmsnorm_add_%s_skip", "rmsnorm_add_%s_skip")
FENCE = 417 * 1829                                         # rows of D = 1408 whose bf16 stream is the first past 2^31 bytes
SHAPES = ((42, 176, 21), (39, 1408, 13), (39, 2560, 13), (21, 4096, 7), (53376, 1408, 417), (10, 4104, 10), (FENCE, 1408, 417),
          (FENCE - 417, 1408, 417))


def _mask(names, present):
    assert set(present) <= set(names), set(present) - set(names)
    return sum(1 << i for i, n in enumerate(names) if n in present)


def _route(L, bwd, flavour, present, M, D, rps):
    """-> dict of the nine fields, or the refusal's message"""
    out = (C.c_int32 * 9)(*([-1] * 9))
    rc = L.ivh_rmsnorm_add_debug_route(bwd, flavour, _mask(BWD_ARGS if bwd else FWD_ARGS, present), M, D, rps, out)
    assert rc in (0, 1)
    if rc:
        return dict(zip(FIELDS, out))
    assert list(out) == [-1] * 9
    return L.ivh_last_error().decode()


def _model(bwd, flavour, present, M, D, rps, bwd_rows=1, cap=512):
    """the rules of the module docstring -> dict of the nine fields, or the text a refusal must carry"""
    skip, bf16 = int(flavour >= 2), flavour & 1
    has = set(present) - (set() if skip else {"branch_slot", "y_slot"}) - ({"dres_extra"} if flavour == PLAIN else set())
    name = ENTRY[flavour] % ("bwd" if bwd else "fwd")
    if M <= 0 or D <= 0 or D % 8:
        return f"{name}: bad shape M={M} D={D}"
    whole = f"{name}: M={M} must be whole samples of {rps} rows"
    nch, n4 = -(-(D // 8) // 64), -(-(D // 8) // 256)
    if not bwd:
        if not has & {"res_in", "branch"}:
            return f"{name}: need res_in or branch"
        if "y" in has and "w" not in has:
            return f"{name}: y requested without weight"
        if skip and (rps <= 0 or M % rps):
            return whole
        if skip and "branch_slot" in has and "res_in" not in has:
            return f"{name}: a compacted branch needs the stream it is added to"
        if not skip and "rowscale" in has and rps <= 0:
            return f"{name}: rows_per_sample must be > 0"
        grid, extra, shmem = min(max(-(-M // 4), 1), 8192), 0, 0
    else:
        if skip and (rps <= 0 or M % rps):
            return whole
        if "dres_extra" in has and skip and not ("dres_out" in has and bf16):
            return f"{name}: dres_extra joins a bf16 dres_out"
        if "dres_extra" in has and "dres_out" not in has:
            return f"{name}: dres_extra joins dres_out (pass it as dres_out when it is the only gradient)"
        if "dbias_part" in has and "dbranch" not in has:
            return f"{name}: dbias_part is the column sum of dbranch"
        if not has & {"dy", "dres_out"}:
            return f"{name}: need dy or dres_out"
        if "dy" in has and not {"res_out", "rstd", "w", "dw_part"} <= has:
            return f"{name}: dy needs res_out, rstd, w, dw_part"
        grid, extra, shmem = min(max(-(-M // 4), 1), cap), int("dres_extra" in has), 16 * D
        if bf16 and set(INTERIOR) <= has and nch <= 8 and bwd_rows != 0 and M * D * 2 < 2 ** 31:
            by_env = (4 if bwd_rows >= 4 else 2 if bwd_rows >= 2 else 1) if n4 == 1 else (2 if bwd_rows >= 2 else 1)
            return dict(zip(FIELDS, (1, n4, 0, 1 if (extra or skip) else by_env, extra, skip, bf16, grid, 0)))
    if nch > 8:
        return f"row width {nch * 512} not supported (max 4096)"
    nch_t, wpr = (nch, 1) if nch <= 4 else (2, 4)
    return dict(zip(FIELDS, (0, nch_t, wpr, 0, extra, skip, bf16, grid, shmem)))


def _bwd_cases():
    """(flavour, present): every flavour x dy or not x tap gradient or not x all ten interior pointers or each one of them missing (dy's own
    absence is the `dy or not` axis: without it its companions rstd / w / res_out / dw_part go too, as ops.rmsnorm_add_bwd calls it)"""
    full = set(INTERIOR) | {"rstd", "w", "rowscale"}
    for flavour, dy, tap, missing in itertools.product(range(4), (1, 0), (0, 1), (None,) + INTERIOR[1:]):
        has = set(full) - ({missing} if missing else set())
        if not dy:
            has -= {"dy", "rstd", "w", "res_out", "dw_part"}
        if tap:
            has |= {"dres_extra"}
        for maps in ((), ("y_slot", "branch_slot")) if flavour >= 2 else ((),):
            yield flavour, frozenset(has | set(maps))


def _fwd_cases():
    for flavour, norm, branch in itertools.product(range(4), (1, 0), (1, 0)):
        has = {"res_in", "res_out"} | ({"w", "y", "rstd"} if norm else set()) | ({"branch", "gamma", "rowscale"} if branch else set())
        for maps in ((), ("y_slot", "branch_slot")) if flavour >= 2 else ((),):
            yield flavour, frozenset(has | set(maps))


def test_route_follows_the_launch_rules_on_the_whole_grid():
    L = lib.load()
    seen = dict(b16=0, generic=0, refused=0, width=set(), n4=set(), capped=0)
    for (M, D, rps), bwd in itertools.product(SHAPES, (0, 1)):
        for flavour, has in (_bwd_cases() if bwd else _fwd_cases()):
            got, want = _route(L, bwd, flavour, has, M, D, rps), _model(bwd, flavour, has, M, D, rps)
            assert got == want, (bwd, flavour, sorted(has), M, D, rps, got, want)
            if isinstance(got, str):
                seen["refused"] += 1
                continue
            seen["b16" if got["b16"] else "generic"] += 1
            if got["b16"]:
                seen["n4"].add(got["nch_t"])
            else:
                seen["width"].add((got["nch_t"], got["wpr"]))
            seen["capped"] += got["grid"] in (512, 8192)
    # the grid reaches both kernels, nch 1 / 3 / 5 / 8 (5 and 8 share <2, 4>), both n4, the grid caps, refusals, and both sides of the size fence
    assert seen["b16"] > 0 and seen["generic"] > 0 and seen["refused"] > 0 and seen["capped"] > 0, seen
    assert seen["width"] == {(1, 1), (3, 1), (2, 4)} and seen["n4"] == {1, 2}, seen
    full = frozenset(set(INTERIOR) | {"rstd", "w"})
    assert _route(L, 1, BF16RES, full, FENCE, 1408, 417)["b16"] == 0 and _route(L, 1, BF16RES, full, FENCE - 417, 1408, 417)["b16"] == 1
    assert "max 4096" in _route(L, 1, BF16RES, full, 10, 4104, 10) and "max 4096" in _route(L, 0, PLAIN, {"res_in", "res_out"}, 10, 4104, 10)
    for nch in (2, 4, 6, 7):                                                       # the widths the grid's shapes leave out
        r = _route(L, 1, PLAIN, full, 16, nch * 512, 4)
        assert (r["nch_t"], r["wpr"]) == ((nch, 1) if nch <= 4 else (2, 4)), (nch, r)


def test_pinned_rows_of_the_headline_step():
    L = lib.load()
    row = lambda *v: dict(zip(FIELDS, v))
    M, D = 128 * 417, 1408
    interior = frozenset(set(INTERIOR) | {"rstd", "w", "rowscale"})
    assert _route(L, 1, BF16RES, interior, M, D, 417) == row(1, 1, 0, 1, 0, 0, 1, 512, 0)                       # a block's interior, bf16 stream
    assert _route(L, 1, BF16RES, interior | {"dres_extra"}, M, D, 417) == row(1, 1, 0, 1, 1, 0, 1, 512, 0)      # a tapped block
    assert _route(L, 1, SKIP_BF16, interior | {"y_slot", "branch_slot"}, M, D, 417) == row(1, 1, 0, 1, 0, 1, 1, 512, 0)
    assert _route(L, 1, SKIP_BF16, interior, M, D, 417) == row(1, 1, 0, 1, 0, 1, 1, 512, 0)                     # skip = the entry, maps or not
    assert _route(L, 1, PLAIN, interior, M, D, 417) == row(0, 3, 1, 0, 0, 0, 0, 512, 22528)                     # fp32 stream: generic
    assert _route(L, 1, PLAIN, interior, M, 3200, 417) == row(0, 2, 4, 0, 0, 0, 0, 512, 51200)                  # the clip decoders' width
    assert _route(L, 1, BF16RES, interior, M, 3200, 417) == row(1, 2, 0, 1, 0, 0, 1, 512, 0)
    assert _route(L, 1, BF16RES, interior - {"gamma", "dgamma_part"}, M, 3200, 417) == row(0, 2, 4, 0, 0, 0, 1, 512, 51200)
    # the first block of the backward pass has no dres_out yet, the last norm no branch: generic
    assert _route(L, 1, BF16RES, interior - {"dres_out"}, M, D, 417)["b16"] == 0
    fwd = frozenset({"res_in", "branch", "gamma", "rowscale", "w", "res_out", "y", "rstd"})
    assert _route(L, 0, BF16RES, fwd, M, D, 417) == row(0, 3, 1, 0, 0, 0, 1, 8192, 0)
    assert _route(L, 0, SKIP_F32, fwd | {"branch_slot", "y_slot"}, M, D, 417) == row(0, 3, 1, 0, 0, 1, 0, 8192, 0)
    assert _route(L, 0, PLAIN, fwd, 7, D, 7) == row(0, 3, 1, 0, 0, 0, 0, 2, 0)


def test_refusals_carry_the_entry_points_own_messages():
    L = lib.load()
    fwd = frozenset({"res_in", "branch", "gamma", "rowscale", "w", "res_out", "y", "rstd"})
    bwd = frozenset(set(INTERIOR) | {"rstd", "w", "rowscale"})
    cases = (
        (0, PLAIN, fwd, 4, 12, 2, "rmsnorm_add_fwd: bad shape M=4 D=12"),                                      # D not a multiple of 8
        (1, BF16RES, bwd, 4, 1412, 2, "rmsnorm_add_bwd_bf16res: bad shape M=4 D=1412"),
        (0, PLAIN, fwd - {"res_in", "branch"}, 4, 16, 2, "rmsnorm_add_fwd: need res_in or branch"),
        (0, BF16RES, fwd - {"w"}, 4, 16, 2, "rmsnorm_add_fwd_bf16res: y requested without weight"),
        (0, PLAIN, fwd, 4, 16, 0, "rmsnorm_add_fwd: rows_per_sample must be > 0"),
        (0, SKIP_BF16, fwd, 10, 16, 3, "rmsnorm_add_fwd_skip: M=10 must be whole samples of 3 rows"),
        (1, SKIP_BF16, bwd, 10, 16, 3, "rmsnorm_add_bwd_skip: M=10 must be whole samples of 3 rows"),
        (1, SKIP_F32, bwd, 10, 16, 0, "rmsnorm_add_bwd_skip: M=10 must be whole samples of 0 rows"),
        (0, SKIP_F32, (fwd - {"res_in"}) | {"branch_slot"}, 4, 16, 2, "rmsnorm_add_fwd_skip: a compacted branch needs the stream it is added to"),
        (1, PLAIN, bwd - {"dbranch"}, 4, 16, 2, "rmsnorm_add_bwd: dbias_part is the column sum of dbranch"),
        (1, SKIP_BF16, bwd - {"dbranch"}, 4, 16, 2, "rmsnorm_add_bwd_skip: dbias_part is the column sum of dbranch"),
        (1, PLAIN, bwd - {"rstd"}, 4, 16, 2, "rmsnorm_add_bwd: dy needs res_out, rstd, w, dw_part"),
        (1, BF16RES, bwd - {"dw_part"}, 4, 16, 2, "rmsnorm_add_bwd_bf16res: dy needs res_out, rstd, w, dw_part"),
        (1, SKIP_F32, bwd - {"res_out"}, 4, 16, 2, "rmsnorm_add_bwd_skip: dy needs res_out, rstd, w, dw_part"),
        (1, BF16RES, bwd - {"dy", "dres_out"}, 4, 16, 2, "rmsnorm_add_bwd_bf16res: need dy or dres_out"),
        (1, SKIP_F32, bwd | {"dres_extra"}, 4, 16, 2, "rmsnorm_add_bwd_skip: dres_extra joins a bf16 dres_out"),        # a tap on an fp32 stream
        (1, SKIP_BF16, (bwd | {"dres_extra"}) - {"dres_out"}, 4, 16, 2, "rmsnorm_add_bwd_skip: dres_extra joins a bf16 dres_out"),
        (1, BF16RES, (bwd | {"dres_extra"}) - {"dres_out"}, 4, 16, 2,
         "rmsnorm_add_bwd_bf16res: dres_extra joins dres_out (pass it as dres_out when it is the only gradient)"),
        (1, PLAIN, bwd, 10, 4104, 10, "row width 4608 not supported (max 4096)"),
        (0, SKIP_BF16, fwd, 10, 4104, 10, "row width 4608 not supported (max 4096)"),
    )
    for b, flavour, has, M, D, rps, text in cases:
        assert _route(L, b, flavour, has, M, D, rps) == text, (b, flavour, sorted(has), M, D, rps)
        assert _model(b, flavour, has, M, D, rps) == text
    # ivh_rmsnorm_add_bwd has no dres_extra argument and only the _skip entries take slot maps: such bits say nothing
    assert _route(L, 1, PLAIN, bwd | {"dres_extra"}, 4, 16, 2) == _route(L, 1, PLAIN, bwd, 4, 16, 2)
    assert _route(L, 0, BF16RES, (fwd - {"res_in"}) | {"branch_slot"}, 4, 16, 2) == _route(L, 0, BF16RES, fwd - {"res_in"}, 4, 16, 2)


_CHILD = """
import ctypes, json, sys
L = ctypes.CDLL(sys.argv[1])
out = (ctypes.c_int32 * 9)()
res = []
for bwd, flavour, mask, M, D, rps in json.loads(sys.argv[2]):
    rc = L.ivh_rmsnorm_add_debug_route(bwd, flavour, ctypes.c_uint32(mask), M, D, rps, out)
    res.append(list(out) if rc == 1 else None)
print(json.dumps(res))
"""


def _child_routes(env, queries):
    """the routes of `queries` in a fresh process (IVH_BWD_ROWS / IVH_BWD_PARTS are read once per process); the library alone, no device"""
    q = [(b, f, _mask(BWD_ARGS if b else FWD_ARGS, has), M, D, rps) for b, f, has, M, D, rps in queries]
    keep = {k: v for k, v in os.environ.items() if k not in ("IVH_BWD_ROWS", "IVH_BWD_PARTS")}
    r = subprocess.run([sys.executable, "-c", _CHILD, lib.LIB_PATH, json.dumps(q)], capture_output=True, text=True, timeout=120, env=dict(keep, **env))
    assert r.returncode == 0, r.stderr
    return [dict(zip(FIELDS, v)) if v else None for v in json.loads(r.stdout)]


def test_bwd_rows_and_bwd_parts_switches_show_in_the_route():
    full = frozenset(set(INTERIOR) | {"rstd", "w", "rowscale"})
    queries = [(1, BF16RES, full, 53376, 1408, 417), (1, BF16RES, full, 53376, 3200, 417), (1, BF16RES, full | {"dres_extra"}, 53376, 1408, 417),
               (1, SKIP_BF16, full, 53376, 1408, 417), (1, PLAIN, full, 53376, 1408, 417), (0, BF16RES, {"res_in", "res_out"}, 53376, 1408, 417),
               (1, BF16RES, full, 100, 1408, 4)]
    for rows, parts, cap in ((0, "1024", 1024), (2, "63", 512), (4, "8193", 512), (None, "64", 64), (3, "8192", 8192), (9, "many", 512)):
        env = dict(IVH_BWD_PARTS=parts, **({} if rows is None else {"IVH_BWD_ROWS": str(rows)}))
        eff = 1 if rows is None or not 0 <= rows <= 4 else rows
        got = _child_routes(env, queries)
        for (b, f, has, M, D, rps), r in zip(queries, got):
            assert r == _model(b, f, has, M, D, rps, bwd_rows=eff, cap=cap), (rows, parts, b, f, sorted(has), M, D, r)
        inner, wide, tapped, skipped, fp32, fwd, small = got
        if rows == 0:
            assert inner["b16"] == wide["b16"] == tapped["b16"] == skipped["b16"] == 0 and inner["shmem_bytes"] == 16 * 1408
        else:
            assert (inner["rows"], wide["rows"]) == {1: (1, 1), 2: (2, 2), 3: (2, 2), 4: (4, 2)}[eff]
            assert tapped["rows"] == skipped["rows"] == 1 and tapped["b16"] == skipped["b16"] == 1
        assert inner["grid"] == fp32["grid"] == cap and fwd["grid"] == 8192 and small["grid"] == 25

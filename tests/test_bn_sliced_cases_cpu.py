"""CPU checks of tests/bn_sliced_cases.py, the references of test_bn_sliced_gpu.py.  (1) Precision: for every case and quantity the float32
evaluation in the kernels' order (16-bit inputs, per-thread accumulation by pixel group, the shuffle / wave tree, fp64 fan-in of fp32 rows,
fp32 coefficient stores, the contracted fma forms of bn_math.h) stays within a QUARTER of the tolerance the kernels get against float64.
(2) Tightness: a partial row dropped, counted twice or replaced by a repeat of the one before, the last pixel of the last group omitted, a
group-boundary pixel attributed to the neighbouring row, a flipped PReLU mask, count - 1 for count, a biased running variance, the
covariance dropped from the derived variance, the third backward statistic read as the second, the neighbouring channel's slope: each
moves at least one quantity beyond its tolerance in every case where it applies.  (3) Conditioning: the special channels are what they
claim, exact ties give z == 0 at both precisions, no other |z| under ZMIN, no 16-bit result under RMIN unless exactly 0, given rows
pairwise different.  (4) Geometry: the mirror against hand-written values; xcd_remap a permutation that keeps a pixel group's slices
on consecutive logical ids."""
import pytest
import torch

import bn_sliced_cases as S

f32, f64 = S.f32, S.f64
S16 = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
QUARTER = 0.25


def _any_exceeds(bad, ref, names, what):
    assert any(S.exceeds(bad[n].value, ref[n]) for n in names), what


def _stored(q, s16):
    return S.r16(q.value.to(f32), s16)


def _rmin(q, what):
    v = q.value
    nz = v[v != 0]
    assert nz.numel() == 0 or float(nz.abs().min()) >= S.RMIN, what


def _largest(score):
    flat = int(score.argmax())
    return flat // score.shape[1], flat % score.shape[1]


def _fwd_specials(c, gamma, rstd):
    if gamma:
        assert c.p.gamma[S.NEG] < 0 and c.p.gamma[S.ZERO] == 0
    x = c.x.to(f64)
    assert abs(float(x[:, S.BIG].mean() / x[:, S.BIG].std()) - 32) < 4
    if getattr(c, "const", True):
        assert bool((c.x[:, S.CONST] == S.CONST_X).all())
        S_ = c.rows.to(f64).sum(0)
        assert float(S_[-1, S.CONST] / c.count - (S_[0, S.CONST] / c.count) ** 2) < 0       # the clamp is needed ...
        assert float(rstd.value[S.CONST]) == 1.0 / S.EPSF ** 0.5                              # ... and gives rstd = 1 / sqrt(eps)


# ================================================================================================ bn_apply_sliced
@pytest.mark.parametrize("s16", S16, ids=IDS)
@pytest.mark.parametrize("key", list(S.FWD_TABLE))
def test_apply_reference(key, s16):
    c = S.case("apply", key, s16)
    try:
        M = c.M
        assert S.sliced_ok(M, c.C, c.P) and S.pairwise_distinct(c.rows), c.name
        cq = c.coef()
        _fwd_specials(c, c.gamma is not None, cq["rstd"])
        names = ["mean", "rstd", "scale", "shift"] + (["rm", "rv"] if c.rm is not None else [])
        for n in names:
            S.check(S.stored32(cq[n]), cq[n], c.name + " " + n + " fp32", QUARTER)
        for what, rows in S.row_variants(c.rows):
            _any_exceeds(c.coef(rows=rows), cq, names, c.name + ": " + what)
        _any_exceeds(c.coef(count=c.count - 1), cq, names, c.name + ": count - 1")
        if c.rm is not None:
            assert S.exceeds(c.coef(unbiased=False)["rv"].value, cq["rv"]), c.name + ": biased running variance"
        sc, sh = S.stored32(cq["scale"]), S.stored32(cq["shift"])
        yq = c.y(sc, sh)
        _rmin(yq, c.name)
        S.check(c.y(sc, sh, f32).value, yq, c.name + " y fp32", QUARTER)
        if c.prelu:
            z, z32 = c.z(sc, sh), c.z(sc, sh, f32)
            live = (sc != 0).expand_as(z)
            assert float(z[live].abs().min()) >= S.ZMIN and torch.equal(z32 > 0, z > 0), c.name
            flip = _largest(z.abs() * live)
            assert S.exceeds(c.y(sc, sh, flip=flip).value, yq), c.name + ": one flipped mask"
            assert S.exceeds(c.y(sc, sh, neighbour_slope=True).value, yq), c.name + ": the neighbouring channel's slope"
        if c.stats:
            y16 = _stored(yq, s16)
            sq = c.stats_q(y16)
            S.check(c.stats_q(y16, f32).value, sq, c.name + " stats fp32", QUARTER)
            assert S.exceeds(c.stats_q(y16, gid=S.gid_last_pixel_lost(M, c.ppg)).value, sq), c.name + ": last pixel omitted"
            assert S.exceeds(c.stats_q(y16, gid=S.gid_boundary_moved(M, c.ppg)).value, sq), c.name + ": boundary pixel in the neighbouring row"
    finally:
        S.drop("apply", key, s16)


# ================================================================================================ bn_apply2_sliced
@pytest.mark.parametrize("s16", S16, ids=IDS)
@pytest.mark.parametrize("key", list(S.APPLY2_TABLE))
def test_apply2_reference(key, s16):
    c = S.case("apply2", key, s16)
    try:
        assert S.apply2_ok(c.M, c.C, c.P) and S.pairwise_distinct(c.rows), c.name
        cq = c.coef()
        _fwd_specials(c, True, cq["rstd"])
        assert c.np.gamma[S.NEG] < 0 and c.np.gamma[S.ZERO] == 0
        n1 = ["mean", "rstd", "scale", "shift", "rm", "rv"]
        n2 = ["nmean", "nrstd", "nscale", "nshift", "nrm", "nrv"]
        for n in n1:
            S.check(S.stored32(cq[n]), cq[n], c.name + " " + n + " fp32", QUARTER)
        sc, sh = S.stored32(cq["scale"]), S.stored32(cq["shift"])
        dq = c.second(sc, sh)
        for n in n2:
            S.check(S.stored32(dq[n]), dq[n], c.name + " " + n + " fp32", QUARTER)
        for what, rows in S.row_variants(c.rows):
            _any_exceeds(c.coef(rows=rows), cq, n1, c.name + ": " + what)
            _any_exceeds(c.second(sc, sh, rows=rows), dq, n2, c.name + ": " + what + " (derived)")
        _any_exceeds(c.coef(count=c.count - 1), cq, n1, c.name + ": count - 1")
        _any_exceeds(c.second(sc, sh, count=c.count - 1), dq, n2, c.name + ": count - 1 (derived)")
        assert S.exceeds(c.coef(unbiased=False)["rv"].value, cq["rv"]) and S.exceeds(c.second(sc, sh, unbiased=False)["nrv"].value, dq["nrv"]), c.name
        _any_exceeds(c.second(sc, sh, with_cov=False), dq, ["nrstd"], c.name + ": cov dropped from ovar")
        oq = c.out(sc, sh)
        _rmin(oq, c.name)
        S.check(c.out(sc, sh, f32).value, oq, c.name + " out fp32", QUARTER)
        o16 = _stored(oq, s16)
        nsc, nsh = S.stored32(dq["nscale"]), S.stored32(dq["nshift"])
        yq = c.y2(o16, nsc, nsh)
        _rmin(yq, c.name)
        S.check(c.y2(o16, nsc, nsh, f32).value, yq, c.name + " y2 fp32", QUARTER)
        mq = c.measured(o16, sc, sh)
        for n in ("nmean", "nrstd"):
            S.check(S.stored32(dq[n]), mq[n], c.name + " derived vs measured " + n, QUARTER)
    finally:
        S.drop("apply2", key, s16)


# ================================================================================================ bn_bwd_sliced
@pytest.mark.parametrize("s16", S16, ids=IDS)
@pytest.mark.parametrize("key", list(S.BWD_TABLE))
def test_bwd_reference(key, s16):
    c = S.case("bwd", key, s16)
    try:
        M, p = c.M, c.p
        assert S.sliced_ok(M, c.C, c.P, True), c.name
        assert p.gamma[S.NEG] < 0 and p.gamma[S.ZERO] == 0 and bool((c.x[:, S.CONST] == S.CONST_X).all())
        x = c.x.to(f64)
        assert abs(float(x[:, S.BIG].mean() / x[:, S.BIG].std()) - 32) < 4
        if c.alpha:
            z = x * p.sc.to(f64) + p.sh.to(f64)
            assert bool(c.keep.any()) and bool((z[c.keep] == 0).all()), c.name
            assert float(z[~c.keep & (p.sc != 0).expand_as(c.keep)].abs().min()) >= S.ZMIN, c.name
            z32 = S.fma(c.x.to(f32), p.sc, p.sh.expand_as(c.x), f32)
            assert bool((z32[c.keep] == 0).all()) and torch.equal(z32 <= 0, z <= 0), c.name
        live = (p.gamma != 0).expand(M, c.C)
        mid = M // 2 + 1
        flip = _largest((c.dy.to(f64).abs() * live)[mid:mid + 1])
        flip = (mid, flip[1])
        names = ["dbeta", "dgamma"] + (["dalpha"] if c.alpha else [])
        if c.rows_in > 0:
            assert S.pairwise_distinct(c.rows, c.nv), c.name
            rows32 = c.rows
        else:
            rq = c.reduce_rows_q()
            rows32 = c.reduce_rows(f32)
            S.check(rows32, rq, c.name + " reduce rows fp32", QUARTER)
            if not c.alpha:
                assert float(rq.value[:, 2].abs().max()) == 0.0
            assert S.exceeds(c.reduce_rows(gid=S.gid_last_pixel_lost(M, c.ppg)), rq), c.name + ": last pixel omitted"
            assert S.exceeds(c.reduce_rows(gid=S.gid_boundary_moved(M, c.ppg)), rq), c.name + ": boundary pixel in the neighbouring row"
            if c.alpha:
                assert S.exceeds(c.reduce_rows(flip=flip), rq), c.name + ": one flipped mask"
                assert S.exceeds(c.reduce_rows(neighbour_slope=True), rq), c.name + ": the neighbouring channel's slope"
        gq = c.grads_q(rows32)
        for n in names:
            S.check(S.stored32(gq[n]), gq[n], c.name + " " + n + " fp32", QUARTER)
        for what, rows in S.row_variants(rows32):
            _any_exceeds(c.grads_q(rows), gq, names, c.name + ": " + what)
        assert S.exceeds(c.grads_q(rows32, second=2)["dgamma"].value, gq["dgamma"]), c.name + ": third statistic read as the second"
        q = c.dx(rows32)
        _rmin(q, c.name)
        if not c.has_add:
            assert float(q.value[~live].abs().max()) == 0.0
        S.check(c.dx(rows32, f32).value, q, c.name + " dx fp32", QUARTER)
        assert S.exceeds(c.dx(rows32, count=c.count - 1).value, q), c.name + ": count - 1"
        assert S.exceeds(c.dx(rows32, second=2).value, q), c.name + ": third statistic read as the second (dx)"
        if M <= 4096:                                          # (the parameter gradients above show these at every size)
            for what, rows in S.row_variants(rows32):
                assert S.exceeds(c.dx(rows).value, q), c.name + ": " + what + " (dx)"
        if c.alpha:
            assert S.exceeds(c.dx(rows32, flip=flip).value, q), c.name + ": one flipped mask (dx)"
            assert S.exceeds(c.dx(rows32, neighbour_slope=True).value, q), c.name + ": the neighbouring channel's slope (dx)"
        if c.has_nx:
            dx16 = _stored(q, s16)
            nq = c.next_rows_q(dx16)
            S.check(c.next_rows_q(dx16, f32).value, nq, c.name + " next rows fp32", QUARTER)
            assert float(nq.value[:, 2].abs().max()) == 0.0 and float(nq.tol[:, 2].abs().max()) == 0.0
            assert S.exceeds(c.next_rows_q(dx16, gid=S.gid_last_pixel_lost(M, c.ppg)).value, nq), c.name + ": last pixel omitted (next rows)"
            assert S.exceeds(c.next_rows_q(dx16, gid=S.gid_boundary_moved(M, c.ppg)).value, nq), c.name + ": boundary pixel (next rows)"
    finally:
        S.drop("bwd", key, s16)


# ================================================================================================ geometry
def test_geometry_mirror():
    """G, ppg, last group size, grid size against the hand-written table; the chosen kernel variants; the fan-in constants"""
    for (M, C), (fw, bw) in S.GEOMETRY.items():
        G, ppg = S.sliced_geometry(M, C)
        assert (G, ppg, M - (G - 1) * ppg, G * (C // 32)) == fw, (M, C)
        G, ppg = S.sliced_geometry(M, C, True)
        assert (G, ppg, M - (G - 1) * ppg) == bw, (M, C)
    assert (S.RG[2], S.RG[3]) == (16, 10) and S.NARROW == {"fwd": 256, "bwd2": 128, "bwd3": 130}
    # NP = 7 up to ppg = 448, 13 beyond; narrow / wide fan-in of apply2 at 130 / 131
    assert S.apply_variant(3584, 1024, True) == "bn_apply_s<NP=7,X2=1>" and S.apply_variant(3585, 1024, False) == "bn_apply_s<NP=13,X2=0>"
    assert S.apply_variant(6657, 1024, True) == "bn_apply_s<NP=13,X2=1>" and S.apply_variant(256, 64, False) == "bn_apply_s<NP=7,X2=0>"
    assert S.apply2_variant(264, 96, 130) == "bn_apply2_s<NP=7,FL=13>" and S.apply2_variant(264, 96, 131) == "bn_apply2_s<NP=7,FL=26>"
    assert S.apply2_variant(3585, 1024, 200) == "bn_apply2_s<NP=13,FL=26>" and S.apply2_variant(3584, 1024, 19) == "bn_apply2_s<NP=7,FL=13>"
    # the (alpha, next, add) variant number and the double fan-in at 128 / 129 rows (two statistics) and 130 / 131 (three)
    assert S.bwd_variant(128, False, False, False)[:2] == (0, 1) and S.bwd_variant(129, False, True, False)[:2] == (2, 2)
    assert S.bwd_variant(130, True, False, True)[:2] == (5, 1) and S.bwd_variant(131, True, True, False)[:2] == (6, 2)
    assert S.bwd_variant(5, True, True, True)[2] == "bn_bwd_apply_s<v=7(alpha,next,add),FX=1>"
    # prefetch / chunk boundaries of the backward kernels
    assert [S.bwd_apply_chunks(p) for p in (8, 192, 200, 264, 320, 328, 840, 1664)] == [0, 0, 1, 1, 1, 2, 6, 12]
    assert [S.bwd_reduce_chunks(p, False) for p in (192, 256, 264)] == [1, 1, 2] and [S.bwd_reduce_chunks(p, True) for p in (128, 136, 192)] == [1, 2, 2]
    # what is served
    assert S.sliced_ok(256, 64, 1) and not S.sliced_ok(255, 64, 1) and S.sliced_ok(13671, 1024, 1) and not S.sliced_ok(13672, 1024, 1)
    assert not any(S.sliced_ok(256, C, 1) for C in (48, 80, 1056)) and not S.sliced_ok(256, 64, 0) and not S.sliced_ok(256, 64, 257)
    assert S.sliced_ok(256, 64, 256, True) and not S.sliced_ok(256, 64, 257, True) and S.apply2_ok(264, 96, 260) and not S.apply2_ok(264, 96, 261)
    for kind, M, C, P in S.REJECT:
        ok = S.apply2_ok(M, C, P) if kind == "apply2" else S.sliced_ok(M, C, P if kind == "apply" else (P or S.sliced_geometry(M, C, True)[0]), kind == "bwd")
        assert not ok, (kind, M, C, P)


def test_table_reaches_every_branch():
    """for every branch the direct tests are there for, a table row whose recorded variant says it is the one launched"""
    bv = {}
    for k, r in S.BWD_TABLE.items():
        G = S.sliced_geometry(r["M"], r["C"], True)[0]
        P = r["rows_in"] or G
        bv.setdefault(S.bwd_variant(P, bool(r["variant"] & 4), bool(r["variant"] & 2), bool(r["variant"] & 1))[:2] + (r["rows_in"] > 0,), []).append(k)
    for v in range(8):
        assert (v, 1, False) in bv and (v, 1, True) in bv, v
    assert (0, 2, True) in bv and (4, 2, True) in bv                         # FX = 2 with and without PReLU
    fi = [S.row_info("apply", k) for k in S.FWD_TABLE]
    bi = [S.row_info("bwd", k) for k in S.BWD_TABLE]
    assert any(i["ppg"] == 832 and i["G"] > 8 and i["last"] == 1 for i in fi)                      # the forward ppg cap, a one-pixel last group
    assert any(i["ppg"] == 1664 and i["last"] == 1 and i["own_rows"] for i in bi)                  # the backward ppg cap
    assert any(i["ppg"] == 448 and i["kernel"].startswith("bn_apply_s<NP=7") for i in fi) and any(i["ppg"] == 456 for i in fi)
    assert any(i["last"] == 1 and i["ppg"] == 8 for i in fi + bi) and any(i["passes"] == 1 and i["last"] == 8 for i in fi + bi)
    # the backward apply pass: exactly its three prefetched passes / one chunk of 8 pixels / the second chunk; the reduce pass: one chunk / two
    own = [i for i in bi if i["own_rows"]]
    assert any(i["ppg"] == 192 and i["apply_chunks"] == 0 for i in own) and any(i["ppg"] == 200 and i["apply_chunks"] == 1 for i in bi)
    assert any(i["ppg"] == 328 and i["apply_chunks"] == 2 for i in own)
    assert any(i["ppg"] == 264 and i["reduce_kernel"] == "bn_bwd_reduce_s<ALPHA=0,U=4>" and i["reduce_chunks"] == 2 for i in own)
    assert any(i["reduce_kernel"] == "bn_bwd_reduce_s<ALPHA=1,U=2>" and i["reduce_chunks"] > 2 for i in own)
    fv = {S.apply_variant(r["M"], r["C"], r.get("x2", False)) for r in S.FWD_TABLE.values()}
    assert fv == {"bn_apply_s<NP=%d,X2=%d>" % (n, x) for n in (7, 13) for x in (0, 1)}
    av = {S.apply2_variant(**r) for r in S.APPLY2_TABLE.values()}
    assert av == {"bn_apply2_s<NP=%d,FL=%d>" % (n, f) for n in (7, 13) for f in (13, 26)}
    grids = {(r["M"], r["C"]): S.GEOMETRY[(r["M"], r["C"])][0][3] for r in S.FWD_TABLE.values()}
    assert grids[(264, 96)] % 8 and grids[(300, 160)] % 8
    assert {r["P"] for r in S.FWD_TABLE.values()} >= set(S.FWD_FANIN) and {r["P"] for r in S.APPLY2_TABLE.values()} >= set(S.APPLY2_FANIN)
    assert {r["rows_in"] for r in S.BWD_TABLE.values() if r["variant"] == 0} >= set(S.BWD_FANIN2)
    assert {r["rows_in"] for r in S.BWD_TABLE.values() if r["variant"] == 4} >= set(S.BWD_FANIN3)
    assert {tuple(r.get("null", ())) for r in S.FWD_TABLE.values()} >= {("gamma",), ("beta",), ("rm",), ("gamma", "beta", "rm")}
    assert {tuple(r["null"]) for r in S.BWD_TABLE.values()} >= {("dgamma",), ("dbeta",), ("dalpha",), ("dgamma", "dbeta", "dalpha")}


def test_xcd_remap_is_a_permutation():
    grids = {g[0][3] for g in S.GEOMETRY.values()}
    assert {99, 190} <= grids and any(g % 8 == 0 for g in grids)
    for (M, C), (fw, _) in S.GEOMETRY.items():
        for grid in {fw[3], S.sliced_geometry(M, C, True)[0] * (C // 32)}:
            lid = [S.xcd_remap(i, grid) for i in range(grid)]
            assert sorted(lid) == list(range(grid)), grid
            # logical id = g * NS + s: the slices of pixel group g are the consecutive ids g NS .. g NS + NS - 1, each reached exactly once
            NS = C // 32
            owners = {}
            for b, l in enumerate(lid):
                owners.setdefault(l // NS, []).append(l % NS)
            assert all(sorted(v) == list(range(NS)) for v in owners.values()) and len(owners) == grid // NS

"""The fine apply streaming the 24-bit copy of the level-0 inverses (csrc/narrow.h;
MAS_INV_WIDE=0, the default) against the fp32 inverses (MAS_INV_WIDE=1), the
oracle, its own documented decode, and every path that rewrites level-0
inverses (a second Prepare, fused and unfused; a blob load; a sharded Prepare).

Bars: rel_err(z_narrow, z_wide) <= 1e-6 -- four times the worst value of the
CPU simulation of the format, so a wrong slot, scale or
sign (1e-2 and up) cannot hide; rel_err(z_narrow, oracle) <= 1e-5, the
project's Z_TOL."""
import dataclasses

import numpy as np
import pytest

from conftest import cloth, tet

pytestmark = pytest.mark.gpu

Z_TOL = 1e-5
NARROW_TOL = 1e-6
NARROW_BLOCK_BYTES = 14272
QMAX = 8388607


def rel_err(a, b):
    return float(np.linalg.norm((a - b)[:, :3].astype(np.float64)) / np.linalg.norm(b[:, :3].astype(np.float64)))


def _handle(monkeypatch, wide, mesh, L, contacts=None, **kw):
    import mas_amd
    monkeypatch.setenv("MAS_INV_WIDE", "1" if wide else "0")
    return mas_amd.from_mesh(mesh, max_levels=L, contacts=contacts, **kw)


def _mesh(kind, W):
    return cloth(W) if kind == "cloth" else tet(W)


def _scaled(mesh, f):
    f = np.float32(f)
    return dataclasses.replace(mesh, diag=(mesh.diag * f).astype(np.float32), off=(mesh.off * f).astype(np.float32))


def _check_narrow_vs_wide(monkeypatch, mesh, L, contacts, seed, tag):
    from mas_amd import meshgen
    r = meshgen.residual(mesh.nV, seed)
    zn = _handle(monkeypatch, False, mesh, L, contacts).Preconditioning(None, r)
    zw = _handle(monkeypatch, True, mesh, L, contacts).Preconditioning(None, r)
    assert np.all(np.isfinite(zn)) and np.all(zn[:, 3] == 0.0)
    e = rel_err(zn, zw)
    print(f"{tag}: rel_err(z_narrow, z_wide) = {e:.3e}")
    assert e <= NARROW_TOL
    return zn, zw


@pytest.mark.parametrize("kind,W,L,nc", [("cloth", 33, 1, 0), ("cloth", 100, 3, 0), ("tet", 16, 4, 0),
                                         ("cloth", 64, 3, 500)])
def test_narrow_against_wide_and_oracle(kind, W, L, nc, monkeypatch):
    from mas_amd import meshgen
    from oracle import Oracle
    mesh = _mesh(kind, W)
    contacts = meshgen.vf_contacts(mesh, nc, seed=3) if nc else None
    zn, zw = _check_narrow_vs_wide(monkeypatch, mesh, L, contacts, 0x5EED, f"{kind}{W} L={L} contacts={nc}")
    o = Oracle(mesh.nV, mesh.edges.shape[0], mesh.faces.shape[0], L, 4)
    o.allocate(mesh)
    if contacts is None:
        o.prepare(mesh)
    else:
        o.prepare(mesh, vf=contacts[0], vfC=contacts[1])
    zo = o.apply(meshgen.residual(mesh.nV, 0x5EED))
    eo, ew = rel_err(zn, zo), rel_err(zw, zo)
    print(f"{kind}{W} L={L} contacts={nc}: rel_err vs oracle narrow {eo:.3e}, wide {ew:.3e}")
    assert eo <= Z_TOL


def _slot_tables():
    """csrc/layout.h in numpy: per packed slot o its (i, j), and for the main
    part its lane record (L, f)."""
    ii, jj = np.zeros(4656, np.int64), np.zeros(4656, np.int64)
    lane = np.full(4656, -1, np.int64)
    for o in range(4656):
        if o < 4608:
            F, comp = o >> 2, o & 3
            q, Ln = F >> 6, F & 63
            h, n, f = Ln >> 5, Ln & 31, 4 * q + comp
            lane[o] = Ln
            if h == 1 or f < 63:
                k, e = divmod(f, 9)
                s = 8 + k if h else 1 + k
                r, c = 3 * n + e // 3, 3 * ((n + s) & 31) + e % 3
            elif f < 66:
                b = f - 63
                r, c = (3 * n, 3 * (n + 16) + b) if n < 16 else (3 * (n - 16) + 1, 3 * n + b)
            else:
                d = f - 66
                a = 0 if d < 3 else (1 if d < 5 else 2)
                b = d if d < 3 else (d - 2 if d < 5 else 2)
                r, c = 3 * n + a, 3 * n + b
        else:
            p, b = divmod(o - 4608, 3)
            r, c = 3 * p + 2, 3 * (p + 16) + b
        ii[o], jj[o] = min(r, c), max(r, c)
    return ii, jj, lane


def _quantise(packed, lane):
    """The rule of narrow.h on [nblk, 4656] packed fp32 inverses: per lane
    record s = fl32(max|x| / 8388607), q = rint(x (1 / s)) in fp64, clamped;
    the tail stays."""
    out = packed.astype(np.float64).copy()
    for Ln in range(64):
        sel = np.nonzero(lane == Ln)[0]
        x = packed[:, sel]
        m = np.abs(x).max(axis=1)
        s = (m / np.float32(QMAX)).astype(np.float32)
        assert np.all((s > 0) | (m == 0)) and np.all(s[s > 0] >= np.finfo(np.float32).tiny), "normal scales expected"
        sd = np.where(s > 0, s, 1.0).astype(np.float64)[:, None]
        q = np.clip(np.rint(x.astype(np.float64) * (1.0 / sd)), -QMAX, QMAX)
        out[:, sel] = (q * sd).astype(np.float32)  # decode: fl32(q s)
    return out


@pytest.mark.parametrize("kind,W", [("cloth", 33), ("tet", 12)])
def test_decode_is_the_documented_one(kind, W, monkeypatch):
    """L = 1: z = Z0, so every block's z is its own matrix times its r.  Block
    by block the narrow apply is as close to the numpy-quantised matrix Q as
    the wide apply is to the fp32 inverse:
    |z_narrow - Q r| <= 1.5 |z_wide - Inv r| + 1e-7 |z_block|."""
    from mas_amd import meshgen
    mesh = _mesh(kind, W)
    r = meshgen.residual(mesh.nV, 91)
    Pn = _handle(monkeypatch, False, mesh, 1)
    Pw = _handle(monkeypatch, True, mesh, 1)
    assert Pn.info()["num_levels"] == 1
    zn, zw = Pn.Preconditioning(None, r), Pw.Preconditioning(None, r)
    nblk = (mesh.nV + 31) // 32
    packed = Pn.packed_inverses(0, nblk)
    assert np.array_equal(packed.view(np.uint32), Pw.packed_inverses(0, nblk).view(np.uint32))
    ii, jj, lane = _slot_tables()
    s2o = Pn.maps()["s2o"]
    for name, P_, z in (("narrow", _quantise(packed, lane), zn), ("wide", packed.astype(np.float64), zw)):
        M = np.zeros((nblk, 96, 96))
        M[:, ii, jj] = P_
        M[:, jj, ii] = P_
        rs = np.zeros((nblk * 32, 3))
        rs[: mesh.nV] = r[s2o, :3]
        want = np.einsum("bij,bj->bi", M, rs.reshape(nblk, 96)).reshape(nblk * 32, 3)
        got = np.zeros((nblk * 32, 3))
        got[: mesh.nV] = z[s2o, :3]
        d = np.linalg.norm((got - want).reshape(nblk, 96), axis=1)
        if name == "narrow":
            dn, zb = d, np.linalg.norm(want.reshape(nblk, 96), axis=1)
        else:
            dw = d
    bar = 1.5 * dw + 1e-7 * zb
    worst = float((dn / bar).max())
    print(f"{kind}{W}: {nblk} blocks, worst |z_narrow - Q r| / bar = {worst:.3f}; "
          f"max |z_narrow - Q r| / |z| = {float((dn / zb).max()):.3e}, "
          f"max |z_wide - Inv r| / |z| = {float((dw / zb).max()):.3e}")
    assert np.all(dn <= bar), int(np.argmax(dn / bar))


@pytest.mark.parametrize("f", [1e6, 1e-6])
def test_scale_invariance(f, monkeypatch):
    """The Hessian times 1e6 and 1e-6: the per-record scale follows the entries,
    the padded last block of cloth(33) (identity rows beside tiny real entries)
    included."""
    _check_narrow_vs_wide(monkeypatch, _scaled(cloth(33), f), 1, None, 5, f"cloth33 L=1 Hessian x {f:g}")


@pytest.mark.parametrize("variant", [None, "2"])
def test_no_stale_copy_after_a_second_prepare(variant, monkeypatch):
    """Prepare, apply, Prepare with other values, apply: bitwise a fresh
    handle's z, on the default (fused) factor and on an unfused one."""
    from mas_amd import meshgen
    if variant is None:
        monkeypatch.delenv("MAS_FACTOR_VARIANT", raising=False)
    else:
        monkeypatch.setenv("MAS_FACTOR_VARIANT", variant)
    mesh = cloth(100)
    other = _scaled(mesh, 1.7)
    r = meshgen.residual(mesh.nV, 13)
    P = _handle(monkeypatch, False, mesh, 3)
    z1 = P.Preconditioning(None, r)
    P.PreparePreconditioner(other.diag, other.off, other.starts)
    z2 = P.Preconditioning(None, r)
    zf = _handle(monkeypatch, False, other, 3).Preconditioning(None, r)
    assert not np.array_equal(z1, z2)
    assert np.array_equal(z2.view(np.uint32), zf.view(np.uint32))


def test_blob_load_rebuilds_the_narrow_copy(monkeypatch):
    import mas_amd
    from mas_amd import meshgen
    mesh = cloth(100)
    r = meshgen.residual(mesh.nV, 17)
    P = _handle(monkeypatch, False, mesh, 3)
    z = P.Preconditioning(None, r)
    Q = mas_amd.SeSchwarzPreconditioner()
    Q.load_blob(P.save_blob())
    assert np.array_equal(Q.Preconditioning(None, r).view(np.uint32), z.view(np.uint32))
    assert Q.info()["device_bytes"] >= Q.info()["num_verts"] // 32 * NARROW_BLOCK_BYTES


def test_shard_prepared_handles_bitwise(monkeypatch):
    """A world of two shard-prepared handles (each narrows only its own
    level-0 blocks): every rank's own rows bitwise the unsharded narrow z."""
    import torch
    import mas_amd
    from mas_amd import meshgen
    mesh = cloth(100)
    monkeypatch.setenv("MAS_INV_WIDE", "0")
    Pf = mas_amd.from_mesh(mesh, max_levels=3)
    r = torch.from_numpy(meshgen.residual(mesh.nV, 6)).cuda()
    s = torch.cuda.Stream()
    z_ref = torch.zeros_like(r)
    torch.cuda.synchronize()
    Pf.PreconditioningDevice(z_ref, r, s.cuda_stream)
    s.synchronize()
    world = 2
    ranks = [mas_amd.from_mesh(mesh, max_levels=3, shard=(g, world)) for g in range(world)]
    mas_amd.exchange_coarse_rows(ranks)
    plans = [Pg.shard_setup(g, world) for g, Pg in enumerate(ranks)]
    seg = plans[0]["seg_max"]
    with torch.cuda.stream(s):
        segs = [torch.zeros((seg, 4), dtype=torch.float32, device="cuda") for _ in range(world)]
        for g, Pg in enumerate(ranks):
            Pg.shard_restrict(g, world, r, segs[g], s.cuda_stream)
        gathered = torch.cat(segs, 0).contiguous()
        z = torch.full_like(r, float("nan"))
        for g, Pg in enumerate(ranks):
            Pg.shard_finish(g, world, gathered, r, z, s.cuda_stream)
    s.synchronize()
    for g, Pg in enumerate(ranks):
        own = torch.from_numpy(Pg.maps()["s2o"][plans[g]["vert_begin"]:plans[g]["vert_end"]].astype(np.int64)).cuda()
        assert torch.equal(z[own], z_ref[own]), g
    assert torch.equal(z, z_ref)


def test_wide_inverse_allocates_no_narrow_copy(monkeypatch):
    """MAS_INV_WIDE=1 (and the wide_inverse keyword): device_bytes smaller by
    exactly the narrow buffer; inv_bytes keeps meaning the fp32 inverses."""
    import mas_amd
    mesh = cloth(64)
    nblk = (mesh.nV + 31) // 32
    n = _handle(monkeypatch, False, mesh, 3).info()
    w = _handle(monkeypatch, True, mesh, 3).info()
    assert n["device_bytes"] - w["device_bytes"] == nblk * NARROW_BLOCK_BYTES
    assert n["inv_bytes"] == w["inv_bytes"] == n["num_blocks"] * 4656 * 4
    monkeypatch.delenv("MAS_INV_WIDE")
    k = mas_amd.from_mesh(mesh, max_levels=3, wide_inverse=True).info()
    assert k["device_bytes"] == w["device_bytes"]

"""The multi-vector apply (mas_apply_multi_device / mas_apply_multi, k_multi.hip):
K residuals through one pass over the inverses give, for every k, bit for bit
the z of a single apply of r[k] on the same handle -- for every level count,
both inverse formats, both level-3 forms, every operand form, the host path, a
restored blob and the C++ facade -- and leave the single-vector path alone."""
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO, cloth, tet

pytestmark = pytest.mark.gpu

KMAX = 8
SHAPES = [("cloth", 100, 3), ("cloth", 256, 4), ("cloth", 33, 1), ("tet", 16, 4)]


def _bits(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _mesh(kind, W):
    return cloth(W) if kind == "cloth" else tet(W)


def _single(P, r):
    """z of one PreconditioningDevice on a side stream, into a zeroed tensor."""
    import torch
    z = torch.zeros_like(r)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    P.PreconditioningDevice(z, r, s.cuda_stream)
    s.synchronize()
    return z


@functools.lru_cache(maxsize=None)
def _case(kind, W, L, cfg=()):
    """One prepared handle per configuration, KMAX residuals (distinct seeds)
    on the device, their single applies on that handle, and one more residual
    with its single apply on a handle of its own (no batch ever ran there)."""
    import torch
    import mas_amd
    from mas_amd import meshgen
    mesh = _mesh(kind, W)
    kw = dict(cfg)
    P = mas_amd.from_mesh(mesh, max_levels=L, **kw)
    r = torch.from_numpy(np.stack([meshgen.residual(mesh.nV, 101 + 7 * k) for k in range(KMAX)])).cuda()
    zs = torch.stack([_single(P, r[k]) for k in range(KMAX)])
    r_mid = torch.from_numpy(meshgen.residual(mesh.nV, 977)).cuda()
    Q = mas_amd.from_mesh(mesh, max_levels=L, **kw)
    z_mid = _single(Q, r_mid)
    del Q
    return dict(mesh=mesh, P=P, r=r, zs=zs, r_mid=r_mid, z_mid=z_mid, L=P.info()["num_levels"])


def _check_batched(kind, W, L, K, cfg=()):
    import torch
    c = _case(kind, W, L, cfg)
    P, r, zs = c["P"], c["r"], c["zs"]
    assert 1 <= c["L"] <= L  # L is max_levels: tet(16) has three natural levels
    s = torch.cuda.Stream()
    zm = torch.zeros(K, c["mesh"].nV, 4, device="cuda")
    torch.cuda.synchronize()
    calls = P.stats()["apply_calls"]
    P.PreconditioningDeviceMulti(zm, r[:K], s.cuda_stream)
    s.synchronize()
    assert P.stats()["apply_calls"] == calls + K
    for k in range(K):
        assert _same(zm[k], zs[k]), f"vector {k} of {K}, first batch"
    # a single apply of another residual in between: the batch left the
    # single-vector coarse scratch alone (the reference z is a fresh handle's) ...
    z_mid = _single(P, c["r_mid"])
    assert _same(z_mid, c["z_mid"])
    rc_mid = P.coarse_residual()
    # ... and the second batch, over the first one's z, is not disturbed by it
    P.PreconditioningDeviceMulti(zm, r[:K], s.cuda_stream)
    s.synchronize()
    for k in range(K):
        assert _same(zm[k], zs[k]), f"vector {k} of {K}, second batch"
    if K > 1:  # (a batch of one is a single apply: mas_capi.h)
        assert _same(P.coarse_residual(), rc_mid)  # mas_get_coarse_residual: still the single apply's


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("kind,W,L", SHAPES)
def test_multi_bitwise_against_single_applies(kind, W, L, K):
    _check_batched(kind, W, L, K)


def test_multi_bitwise_two_levels():
    """L = 2: level 1 alone above the level-0 blocks (one coarse launch, one prolongation term)."""
    assert _case("cloth", 100, 2)["L"] == 2
    _check_batched("cloth", 100, 2, 3)


def test_level_counts_covered():
    """The shapes above reach L = 1, 3 and 4 (and 2 just above): what the kernels template on."""
    assert {_case(*shape)["L"] for shape in SHAPES} == {1, 3, 4}


@pytest.mark.parametrize("cfg", [(("wide_inverse", True),), (("reference_restriction", True),)],
                         ids=["wide_inverse", "reference_restriction"])
def test_multi_bitwise_other_forms(cfg):
    _check_batched("cloth", 256, 4, 3, cfg)


def test_operand_forms():
    """Separately allocated tensors and raw pointers give the bits of the
    [K, nV, 4] tensor; one residual passed twice gives two identical z."""
    import torch
    c = _case("cloth", 100, 3)
    P, r, zs, nV = c["P"], c["r"], c["zs"], c["mesh"].nV
    K = 3
    s = torch.cuda.Stream()
    zl = [torch.zeros(nV, 4, device="cuda") for _ in range(K)]
    rl = [r[k].clone() for k in range(K)]
    torch.cuda.synchronize()
    P.PreconditioningDeviceMulti(zl, rl, s.cuda_stream)
    s.synchronize()
    for k in range(K):
        assert _same(zl[k], zs[k]), k
    zp = torch.zeros(K, nV, 4, device="cuda")
    torch.cuda.synchronize()
    P.PreconditioningDeviceMulti([zp[k].data_ptr() for k in range(K)], [t.data_ptr() for t in rl], s.cuda_stream)
    s.synchronize()
    for k in range(K):
        assert _same(zp[k], zs[k]), k
    z2 = torch.zeros(2, nV, 4, device="cuda")
    torch.cuda.synchronize()
    P.PreconditioningDeviceMulti(z2, [rl[1], rl[1]], s.cuda_stream)
    s.synchronize()
    assert _same(z2[0], zs[1]) and _same(z2[1], zs[1])


def test_host_path():
    c = _case("cloth", 100, 3)
    P, K = c["P"], 3
    r = c["r"][:K].cpu().numpy()
    z = P.PreconditioningMulti(None, r)
    assert z.shape == r.shape and z.dtype == np.float32
    for k in range(K):
        assert _same(z[k], P.Preconditioning(None, r[k])), k
        assert _same(z[k], c["zs"][k]), k
    out = np.zeros_like(r)
    assert P.PreconditioningMulti(out, r) is out
    assert _same(out, z)


def test_restored_blob_serves_the_batch():
    import torch
    import mas_amd
    c = _case("cloth", 100, 3)
    K, nV = 4, c["mesh"].nV
    Q = mas_amd.SeSchwarzPreconditioner()
    Q.load_blob(c["P"].save_blob())
    s = torch.cuda.Stream()
    zm = torch.zeros(K, nV, 4, device="cuda")
    torch.cuda.synchronize()
    Q.PreconditioningDeviceMulti(zm, c["r"][:K], s.cuda_stream)
    s.synchronize()
    for k in range(K):
        assert _same(zm[k], c["zs"][k]), k


def test_refusals():
    """Every malformed batch is refused with its status before anything is
    queued, and the handle serves a valid batch afterwards."""
    import torch
    import mas_amd
    from mas_amd import MasError, _ptr_array
    c = _case("cloth", 100, 3)
    P, r, zs, mesh = c["P"], c["r"], c["zs"], c["mesh"]
    nV, L = mesh.nV, mas_amd.lib()
    z = torch.zeros(3, nV, 4, device="cuda")
    zp, rp = [z[k].data_ptr() for k in range(3)], [r[k].data_ptr() for k in range(3)]
    torch.cuda.synchronize()

    def c_call(h, count, zptrs, rptrs):
        return L.mas_apply_multi_device(h, count, _ptr_array(zptrs), _ptr_array(rptrs), None)

    with pytest.raises(MasError, match="MAS_ERR_ARG"):
        P.PreconditioningDeviceMulti([], [])
    with pytest.raises(MasError, match="MAS_ERR_ARG"):
        P.PreconditioningDeviceMulti(torch.zeros(9, nV, 4, device="cuda"), torch.zeros(9, nV, 4, device="cuda"))
    with pytest.raises(MasError, match="MAS_ERR_ARG"):
        P.PreconditioningDeviceMulti(z, r[:2])  # K of z != K of residual
    # the C ABI's own count check (the binding refuses these before the call)
    assert c_call(P.h, 0, zp, rp) == -1 and b"count" in L.mas_last_error(P.h)
    assert c_call(P.h, 9, zp * 3, rp * 3) == -1 and b"count" in L.mas_last_error(P.h)
    with pytest.raises(MasError, match=r"MAS_ERR_ARG.*z\[0\] is z\[1\]"):
        P.PreconditioningDeviceMulti([z[0], z[0]], [r[0], r[1]])
    with pytest.raises(MasError, match=r"MAS_ERR_ARG.*z\[0\] is r\[1\]"):
        P.PreconditioningDeviceMulti([z[1], z[0]], [r[0], z[1]])
    with pytest.raises(MasError, match="MAS_ERR_ARG.*null"):
        P.PreconditioningDeviceMulti([zp[0], 0], rp[:2])
    with pytest.raises(MasError, match="MAS_ERR_ARG.*aligned"):
        P.PreconditioningDeviceMulti([zp[0], zp[1] + 4], rp[:2])
    U = mas_amd.SeSchwarzPreconditioner()  # never prepared
    with pytest.raises(MasError, match="MAS_ERR_STATE"):
        U.PreconditioningDeviceMulti(z, r[:3])
    assert c_call(U.h, 3, zp, rp) == -4
    S = mas_amd.from_mesh(mesh, max_levels=3, shard=(0, 2))
    with pytest.raises(MasError, match="MAS_ERR_STATE.*one shard"):
        S.PreconditioningDeviceMulti(z, r[:3])
    with pytest.raises(MasError, match="MAS_ERR_STATE"):
        S.PreconditioningMulti(None, r[:3].cpu().numpy())
    torch.cuda.synchronize()
    assert not z.any()  # nothing was queued by any of them
    s = torch.cuda.Stream()
    P.PreconditioningDeviceMulti(z, r[:3], s.cuda_stream)
    s.synchronize()
    for k in range(3):
        assert _same(z[k], zs[k]), k


def test_cpp_facade_multi(tmp_path):
    import mas_amd
    from mas_amd import meshgen
    mesh = cloth(64)
    arrays = [("pos", mesh.pos), ("starts", mesh.starts), ("idx", mesh.idx), ("diag", mesh.diag), ("off", mesh.off)]
    arrays += [(f"r{k}", meshgen.residual(mesh.nV, 211 + k)) for k in range(3)]
    for name, arr in arrays:
        np.ascontiguousarray(arr).tofile(tmp_path / f"{name}.bin")
    exe = tmp_path / "facade_multi"
    lib = os.path.dirname(mas_amd.FACADE_PATH)
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "cpp", "facade_multi.cpp"), "-L", lib, "-lSeSchwarzPreconditioner",
                    "-lmas_amd", f"-Wl,-rpath,{lib}", "-o", str(exe)], check=True)
    p = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "multi_nonzero 1" in p.stdout, p.stdout
    assert "multi_alias_refused 1" in p.stdout, p.stdout
    assert "multi_bitwise 1" in p.stdout, p.stdout

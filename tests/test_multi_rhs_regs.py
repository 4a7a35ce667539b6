"""Register budget of the multi-RHS kernels (csrc/mvec.hip, spmm.hip, gcr_multi.hip) on the code object hipcc builds for gfx950
(-Rpass-analysis=kernel-resource-usage); no GPU needed.  No instantiation may spill to scratch — for k <= 8 that is the
contract, and DESIGN.md section 9 states 0 bytes for the k = 12, 16 forms too — and each reaches the occupancy (waves per
SIMD) written in DESIGN.md section 9, so a change that halves it fails here."""
import os
import re
import shutil
import subprocess

import pytest

CS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mgpreconditionedgcr_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# kernel -> waves per SIMD ("Registers and occupancy")
OCC = {
    # block BLAS-1 <KC columns per thread>
    "mv_dot_kernel<1>": 8, "mv_dot_kernel<2>": 8, "mv_dot_kernel<4>": 8,
    "mv_axpy_kernel<1>": 8, "mv_axpy_kernel<2>": 8, "mv_axpy_kernel<4>": 8,
    # ELL slab, complex values <K, MASK, REALV>
    "ell_multi_kernel<1, false, false>": 8, "ell_multi_kernel<2, false, false>": 8, "ell_multi_kernel<4, false, false>": 5,
    "ell_multi_kernel<4, true, false>": 6, "ell_multi_kernel<8, false, false>": 4, "ell_multi_kernel<8, true, false>": 4,
    "ell_multi_kernel<12, false, false>": 4, "ell_multi_kernel<16, false, false>": 3,
    "ell_multi_kernel<12, true, false>": 3, "ell_multi_kernel<16, true, false>": 2,
    # ... real values
    "ell_multi_kernel<1, false, true>": 8, "ell_multi_kernel<2, false, true>": 8, "ell_multi_kernel<4, false, true>": 8,
    "ell_multi_kernel<8, false, true>": 4, "ell_multi_kernel<8, true, true>": 4, "ell_multi_kernel<12, false, true>": 3,
    "ell_multi_kernel<16, false, true>": 2, "ell_multi_kernel<4, true, true>": 8,
    "ell_multi_kernel<12, true, true>": 3, "ell_multi_kernel<16, true, true>": 2,
    # CSR tail <K>
    "tail_chunk_multi_kernel<2>": 8, "tail_chunk_multi_kernel<4>": 7, "tail_chunk_multi_kernel<8>": 4,
    "tail_long_multi_kernel<2>": 8, "tail_long_multi_kernel<4>": 8, "tail_long_multi_kernel<8>": 6, "tail_long_multi_kernel<16>": 3,
    # dictionary / stencil view <MODE, NS, RARE>
    "rowgen_multi_kernel<1, 0, false>": 8, "rowgen_multi_kernel<2, 0, false>": 7, "rowgen_multi_kernel<3, 7, false>": 8,
    "rowgen_multi_kernel<3, 9, false>": 7, "rowgen_multi_kernel<3, 9, true>": 6,
    # block-CSR <TT>
    "bcsr_multi_kernel<0>": 8, "bcsr_multi_kernel<1>": 8, "bcsr_multi_kernel<2>": 8, "bcsr_multi_kernel<4>": 8,
    "bcsr_multi_kernel<8>": 6, "bcsr_multi_kernel<16>": 3,
    # batched GCR <KC columns per thread> (1024-thread workgroups: 4 .. 7 = one workgroup per CU, 8 = two)
    "m_init_partials_kernel<1, false>": 8, "m_init_partials_kernel<2, false>": 8, "m_init_partials_kernel<4, false>": 4,
    "m_xr_kernel<1>": 8, "m_xr_kernel<2>": 8, "m_xr_kernel<4>": 8,
    "m_dot_kernel<1, 2>": 8, "m_dot_kernel<2, 2>": 8, "m_dot_kernel<4, 2>": 5,
    "m_build_kernel<1, false>": 8, "m_build_kernel<2, false>": 8, "m_build_kernel<4, false>": 4,
    "m_close_x_kernel<1, false>": 8, "m_close_x_kernel<2, false>": 8, "m_close_x_kernel<4, false>": 6,
    "m_pending_x_kernel<1, XFlush>": 8, "m_pending_x_kernel<2, XFlush>": 8, "m_pending_x_kernel<4, XFlush>": 8,
}


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc is not installed")
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    res = {}
    for src in ("mvec.hip", "spmm.hip", "gcr_multi.hip"):
        out = tmp_path_factory.mktemp("regs") / (src + ".o")
        err = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
                              "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(out)],
                             capture_output=True, text=True, cwd=CS, check=True).stderr
        cur = None
        for line in err.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = subprocess.check_output(["c++filt", m.group(1)], text=True).strip()
                cur = re.sub(r"\(.*", "", name).replace("void mgcr::", "").replace("mgcr::", "")
                res[cur] = {}
                continue
            for key in ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]"):
                m = re.search(re.escape(key) + r": (\d+)", line)
                if m and cur:
                    res[cur][key] = int(m.group(1))
    return res


def test_no_multi_rhs_kernel_spills(usage):
    assert len(usage) >= len(OCC)
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0, (name, u)


@pytest.mark.parametrize("kernel", sorted(OCC))
def test_multi_rhs_kernel_occupancy(usage, kernel):
    assert kernel in usage, sorted(usage)
    assert usage[kernel]["Occupancy [waves/SIMD]"] == OCC[kernel], (kernel, usage[kernel])


@pytest.mark.parametrize("K", [2, 4, 8])
def test_tail_chunk_kernel_lds(usage, K):
    """the k-wide chunk kernel stages K products for each of its 256 entries per trip: 16 * K * 256 bytes"""
    assert usage["tail_chunk_multi_kernel<%d>" % K]["LDS Size [bytes/block]"] == 16 * K * 256

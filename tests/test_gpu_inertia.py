"""The certificate of the few-eigenpairs path: #{lambda < vu} from the inertia of C - vu I
(banded L S L^T; csrc/eig2.hip) against LAPACK's eigenvalues, on both kernels (band resident in
LDS; wide bands in place with save / restore), and the planted-eigenvalue case the uncertified
iteration misses.  Reference semantics: dsygvx range 'V' = dstebz Sturm counts,
amg/src/xpacks.cpp:226-288."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sla

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _banded_spsd(n, bw, rng, shift=0.0):
    """Graph-Laplacian-like banded SPSD matrix (null vector = ones) plus shift * diag(rand)."""
    A = np.zeros((n, n))
    for d in range(1, bw + 1):
        w = rng.random(n - d) * (rng.random(n - d) < min(1.0, 6.0 / bw))
        if d == bw:
            w[0] = 1.0          # the band is exactly bw wide
        A[np.arange(n - d), np.arange(d, n)] = -w
    A = A + A.T
    A -= np.diag(A.sum(axis=1))
    A += shift * np.diag(rng.random(n))
    return A


def _snd_D(A):
    d = np.diag(A)
    return (np.abs(A) * np.sqrt(d[:, None] / d[None, :])).sum(axis=1)


@pytest.mark.parametrize("bw", [3, 20, 51, 64, 100, 150, 400])
def test_inertia_counts_match_lapack(bw):
    """bands up to 112 take the LDS kernel (windows 68 / 80 / 128), wider ones the in-place path"""
    from saamge_amd import capi
    rng = np.random.default_rng(bw)
    sizes = [bw + 2, 97, 200, 405, 421] + ([900] if bw > 112 else [])
    mats, diags = [], []
    for n in sizes:
        n = max(n, bw + 2, 64)
        A = _banded_spsd(n, bw, rng, shift=1e-3 if n % 2 else 0.0)
        A += np.diag(np.where(np.diag(A) <= 0, 1.0, 0.0))
        mats.append(A)
        diags.append(_snd_D(A))
    for vu in [0.003, 0.05, 0.3]:
        neg = capi.inertia_batched(mats, diags, vu)
        for A, D, k in zip(mats, diags, neg):
            w = sla.eigh(A, np.diag(D), eigvals_only=True)
            ref = int(np.sum(w < vu))
            gap = np.min(np.abs(w - vu))
            assert k == ref or (k == -1 and gap < 1e-6), (A.shape, bw, vu, k, ref, gap)
        assert np.sum(neg < 0) <= 1      # "not certifiable" must stay the exception


def test_matrices_restored_after_wide_band_inertia():
    """the in-place inertia pass saves and restores the band: the eigenpairs that follow are those of the
    original matrices"""
    from saamge_amd import capi
    rng = np.random.default_rng(5)
    mats = [_banded_spsd(n, 200, rng) for n in (500, 777)]
    diags = [_snd_D(A) for A in mats]
    res = capi.lower_eigens_batched(mats, diags, -1.0, 0.01)
    for A, D, (w, X) in zip(mats, diags, res):
        wr = sla.eigh(A, np.diag(D), eigvals_only=True)
        k = max(1, int(np.sum(wr <= 0.01)))
        assert len(w) == k and np.allclose(w, wr[:k], atol=1e-11)
        R = A @ X - (D[:, None] * X) * w[None, :]
        assert np.abs(R).max() <= 1e-10


_PLANTED = r"""
import sys, numpy as np
sys.path.insert(0, %r)
from saamge_amd import capi

def unit_rand(a, b):            # csrc/eig_device.h unit_rand
    M = 0xFFFFFFFF
    h = ((a * 2654435761) & M) ^ ((b + 0x9e3779b9 + ((a << 6) & M) + (a >> 2)) & M)
    h ^= h >> 16; h = (h * 0x85ebca6b) & M; h ^= h >> 13; h = (h * 0xc2b2ae35) & M; h ^= h >> 16
    return (h + 0.5) * (2.0 / 4294967296.0) - 1.0

n = 96
# the start block of the iteration for D = I: column 0 = ones, columns 1..7 pseudo-random
X0 = np.array([[1.0 if j == 0 else unit_rand(r * 8 + j, n) for j in range(8)] for r in range(n)])
Q, _ = np.linalg.qr(np.concatenate([X0, np.random.default_rng(1).standard_normal((n, n - 8))], axis=1))
# eigenvectors: Q[:, 0] ~ ones (lambda = 0), Q[:, 8] orthogonal to the whole start block (planted, lambda = 0.002),
# everything else far above the window
lam = np.linspace(0.6, 1.0, n)
lam[0] = 0.0
lam[8] = 0.002
C = (Q * lam) @ Q.T
C = 0.5 * (C + C.T)
w, X = capi.lower_eigens_batched([C], [np.ones(n)], -1.0, 0.003)[0]
print("COUNT", len(w))
"""


def test_planted_eigenvalue_orthogonal_to_start_block():
    """An eigenvalue inside the window whose eigenvector is orthogonal to the iteration's start block:
    the iteration converges on everything else first.  With the inertia certificate the result is the
    full count (2); without it (saamge_amd_options.eig_certify = 0, kept for this test) the miss is shown."""
    code = _PLANTED % ROOT
    env = dict(os.environ, SAAMGE_AMD_TEST_OPTIONS="eig_min_n=0")
    o = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert o.returncode == 0, o.stdout + o.stderr
    assert "COUNT 2" in o.stdout, o.stdout + o.stderr
    o2 = subprocess.run([sys.executable, "-c", code], env=dict(env, SAAMGE_AMD_TEST_OPTIONS="eig_min_n=0,eig_certify=0"),
                        capture_output=True, text=True, timeout=300)
    print("uncertified run:", o2.stdout.strip(), o2.stderr.strip()[-300:])
    assert o2.returncode == 0


_RESHIFT = r"""
import sys, numpy as np, scipy.linalg as sla
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from saamge_amd import capi
from test_gpu_inertia import _banded_spsd, _snd_D
rng = np.random.default_rng(11)
mats, diags = [], []
for n in (1400, 1500):
    A = _banded_spsd(n, 150, rng) + 100.0 * np.eye(n)    # every eigenvalue far above the window, the lowest ones close together
    mats.append(A); diags.append(_snd_D(A))
res = capi.lower_eigens_batched(mats, diags, -1.0, 1e-4)
for A, D, (w, X) in zip(mats, diags, res):
    wr = sla.eigh(A, np.diag(D), eigvals_only=True, subset_by_index=[0, 1])
    assert len(w) == 1, len(w)
    assert abs(w[0] - wr[0]) <= 1e-11, (w[0], wr[0])
    R = A @ X - (D[:, None] * X) * w[None, :]
    assert np.abs(R).max() <= 1e-10, np.abs(R).max()
    assert abs(float(X[:, 0] @ (D * X[:, 0])) - 1.0) <= 1e-10
print("OK")
"""


def test_slow_wide_band_matrix_is_factored_again_at_a_better_shift():
    """Wide-band matrices (in-place factorisation through HBM) without an eigenvalue in the window and with their
    lowest eigenvalues close together: at the first shift (just below the window) the smallest pair converges like
    0.8^k; the iteration asks for a shift just below the smallest Ritz value, the batch is factored again and
    finishes on the few-eigenpairs path (STRICT: the dense fallback is an error) with LAPACK's smallest pair."""
    code = _RESHIFT % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, SAAMGE_AMD_TEST_OPTIONS="eig_strict=1,debug=1")
    o = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert o.returncode == 0 and "OK" in o.stdout, o.stdout[-2000:] + o.stderr[-3000:]
    assert "factored again" in o.stderr, o.stderr[-3000:]

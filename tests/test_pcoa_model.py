"""The numpy model of principal coordinates (pcoa_model.py) against what it must mean, and the inputs of the GPU tests."""
import numpy as np
import pytest

import pcoa_model as P


@pytest.mark.parametrize("n,dim,k", [(40, 5, 3), (12, 2, 2), (100, 8, 8)])
def test_points_in_euclidean_space_come_back_as_their_centred_pca_coordinates(n, dim, k):
    rng = np.random.default_rng(n)
    x = rng.standard_normal((n, dim)) * np.arange(dim, 0, -1)
    d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
    eig, coords, trace = P.pcoa(d, k)
    xc = x - x.mean(axis=0)
    u, s, _ = np.linalg.svd(xc, full_matrices=False)
    pca = u[:, :k] * s[:k]
    assert np.allclose(eig, s[:k] ** 2, rtol=1e-10)
    assert np.isclose(trace, (xc ** 2).sum(), rtol=1e-10)
    for a in range(k):
        sign = 1.0 if coords[:, a] @ pca[:, a] > 0 else -1.0
        assert np.allclose(sign * coords[:, a], pca[:, a], atol=1e-8 * s[0])
        assert coords[int(np.argmax(np.abs(coords[:, a]))), a] > 0
    # the distances of the coordinates are the distances given, once every dimension is kept
    if k == dim:
        back = np.sqrt(((coords[:, None, :] - coords[None, :, :]) ** 2).sum(-1))
        assert np.allclose(back, d, atol=1e-8 * d.max())


def test_axes_beyond_n_minus_1_and_non_positive_eigenvalues_are_zero():
    eig, coords, _ = P.pcoa(P.non_euclidean(3, 0), 16)
    assert eig[0] > 0 and abs(eig[1]) < 1e-12 * eig[0] and np.all(eig[2:] == 0) and np.all(coords[:, 2:] == 0)
    eig, coords, _ = P.pcoa(P.line(9, 1), 3)
    assert eig[0] > 0 and np.all(np.abs(eig[1:]) < 1e-12 * eig[0])


@pytest.mark.parametrize("n", [15, 16, 17, 65, 257])
@pytest.mark.parametrize("k", [1, 3, 16])
def test_the_non_euclidean_input_has_a_negative_eigenvalue_larger_than_the_kth(n, k):
    lam = P.spectrum(P.non_euclidean(n, P.SEEDS["non_euclidean"][n]))
    assert -lam[-1] > lam[min(k, n - 1) - 1] > -1e-9 * lam[0]
    assert -lam[-1] > lam[0]                                                                    # larger even than the first
    assert P.spectrum(P.euclidean(n, P.SEEDS["non_euclidean"][n]))[-1] > -1e-9 * lam[0]                                   # the input it was made from has none


@pytest.mark.parametrize("n", [65, 257])
def test_the_diagonal_input_has_more_large_negative_eigenvalues_than_spare_vectors(n):
    lam = P.spectrum(P.diagonal_negative(n, P.SEEDS["diagonal_negative"][n]))
    assert lam[2] > 0.05 * lam[0] and np.sum(-lam > 4 * lam[2]) == 9 and np.all(np.abs(lam[3:-9]) < 1e-9 * lam[0])

"""Host math of the feature-space PCA (aldi_amd/featurespace.py): (sum, gram, count) -> components / explained variance / mean against
scikit-learn's PCA and a numpy SVD restatement, the sign rule, the degenerate counts and the tool's choice of source and target."""
import numpy as np
import pytest

N_ROWS, C = 2000, 256
TOL = 1e-8      # covariance noise is n * 2^-53-scale, the eigen-gap after component 2 is >= 3 in variance: orders below this bound


def planted(n=N_ROWS, c=C, seed=0):
    """X = Z diag(3, 2, 0.5, 0.5 U(0,1) ...) Q + offset: variances 9, 4, then <= 0.25"""
    rng = np.random.RandomState(seed)
    scale = np.concatenate([[3.0, 2.0, 0.5], 0.5 * rng.uniform(0.0, 1.0, c - 3)])
    q, _ = np.linalg.qr(rng.standard_normal((c, c)))
    return (rng.standard_normal((n, c)) * scale) @ q + 0.25 * rng.standard_normal(c)


def svd_pca(x, k=2):
    """numpy restatement of sklearn.decomposition.PCA(k, svd_solver="full") with svd_flip(u_based_decision=False)"""
    mean = x.mean(axis=0)
    _, s, vt = np.linalg.svd(x - mean, full_matrices=False)
    signs = np.sign(vt[np.arange(vt.shape[0]), np.abs(vt).argmax(axis=1)])
    vt = vt * signs[:, None]
    var = s ** 2 / (x.shape[0] - 1)
    return vt[:k], var[:k] / var.sum(), mean


@pytest.fixture(scope="module")
def data():
    x = planted()
    return x, x.sum(axis=0), x.T @ x


def test_pca_from_moments_matches_numpy_svd_and_sklearn(data):
    from aldi_amd.featurespace import pca_from_moments
    x, s, g = data
    res = pca_from_moments(s, g, x.shape[0])
    comp, evr, mean = svd_pca(x)
    errs = {"components": np.abs(res["components"] - comp).max(), "evr": np.abs(res["explained_variance_ratio"] - evr).max(),
            "mean": np.abs(res["mean"] - mean).max()}
    print("vs numpy svd:", errs)
    assert max(errs.values()) <= TOL, errs
    assert res["components"].shape == (2, C) and res["count"] == N_ROWS
    assert np.abs(res["components"] @ res["components"].T - np.eye(2)).max() < 1e-12
    assert res["explained_variance_ratio"][0] > res["explained_variance_ratio"][1] > 0


def test_pca_from_moments_matches_sklearn(data):
    skd = pytest.importorskip("sklearn.decomposition")
    from aldi_amd.featurespace import pca_from_moments
    x, s, g = data
    res = pca_from_moments(s, g, x.shape[0])
    ref = skd.PCA(2, svd_solver="full").fit(x)
    errs = {"components": np.abs(res["components"] - ref.components_).max(),
            "evr": np.abs(res["explained_variance_ratio"] - ref.explained_variance_ratio_).max(), "mean": np.abs(res["mean"] - ref.mean_).max()}
    print("vs sklearn:", errs)
    assert max(errs.values()) <= TOL, errs
    # and the projection the device computes is sklearn's transform
    y = (x - res["mean"]) @ res["components"].T
    assert np.abs(y - ref.transform(x)).max() <= 1e-8 * np.abs(y).max() + TOL


def test_sign_rule_is_independent_of_row_order_and_global_sign(data):
    from aldi_amd.featurespace import pca_from_moments
    x, s, g = data
    res = pca_from_moments(s, g, x.shape[0])
    comp = res["components"]
    top = np.abs(comp).argmax(axis=1)
    assert (comp[np.arange(2), top] > 0).all()
    perm = np.random.RandomState(1).permutation(x.shape[0])
    xp = x[perm]
    res_p = pca_from_moments(xp.sum(axis=0), xp.T @ xp, x.shape[0])
    assert np.abs(res_p["components"] - comp).max() <= TOL
    xm = 2.0 * x.mean(axis=0) - x                        # the data set mirrored about its mean: same components, same signs
    res_m = pca_from_moments(xm.sum(axis=0), xm.T @ xm, x.shape[0])
    assert np.abs(res_m["components"] - comp).max() <= TOL


@pytest.mark.parametrize("n", [0, 1])
def test_too_few_rows_raise_the_named_error(n):
    from aldi_amd.featurespace import FeatureSpaceError, moments_to_mean_cov, pca_from_moments
    x = planted(4, 8)[:n]
    with pytest.raises(FeatureSpaceError, match="at least two"):
        pca_from_moments(x.sum(axis=0), x.T @ x, n)
    with pytest.raises(FeatureSpaceError):
        moments_to_mean_cov(x.sum(axis=0), x.T @ x, n)
    assert issubclass(FeatureSpaceError, ValueError)


def test_moments_to_mean_cov_is_numpy_cov():
    from aldi_amd.featurespace import moments_to_mean_cov
    x = planted(300, 16, seed=3)
    mean, cov, n = moments_to_mean_cov(x.sum(axis=0), x.T @ x, 300)
    assert n == 300 and np.abs(mean - x.mean(axis=0)).max() < 1e-13
    assert np.abs(cov - np.cov(x, rowvar=False)).max() < 1e-11 and (cov == cov.T).all()


def test_dataset_selection_rule():
    from aldi_amd.featurespace import select_datasets
    assert select_datasets((), ("cityscapes_val", "foggy_val")) == ("cityscapes_val", "foggy_val")
    assert select_datasets(("a", "b"), ("s", "t")) == ("s", "t")                 # two test names win whatever TRAIN holds
    assert select_datasets(("cityscapes_train",), ("foggy_val",)) == ("cityscapes_train", "foggy_val")
    for train, test in (((), ()), ((), ("t",)), (("a", "b"), ("t",)), (("a",), ()), (("a",), ("t", "u", "v"))):
        with pytest.raises(ValueError, match="Ambiguous"):
            select_datasets(train, test)

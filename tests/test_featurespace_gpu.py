"""Device feature-space PCA: csrc/featstat.hip (pool_rows, moments_accum, project2) against fp64 host references on the SAME operands,
RCNN.feature_pass against the engine's own intermediates and the oracle, the collector and the tool end to end.

Bounds (u32 = 2^-24, u64 = 2^-53):
* pool_rows avg: S * u32 * max|x| -- the worst case of an fp32 sum of S terms (any order) plus the rounded division; max: exact.
* moments_accum: n * u64 * (|X|^T |X|) elementwise (sum: n * u64 * sum|X|) -- every product is exact in fp64 and no term passes through
  more than n - 1 additions in the two-level ordered reduction.
* project2: 1e-6 * max|Y| -- the fp32 rounding of the output plus a 256-term fp64 dot.
* feature_pass vs the oracle (resnet_fpn -> roi_pool on the device's proposals -> mean; the image level: p6 -> mean): the largest absolute
  difference measured once in fp32 mode on the MI355X (ORACLE_MEASURED_PROP / ORACLE_MEASURED_IMG, also in DESIGN section 19; the test
  prints both on every run), asserted at 4x and never looser than the project's parity bound 1e-3 * max|x|.
"""
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
K, H, W = 8, 192, 256
U32, U64 = 2.0 ** -24, 2.0 ** -53
# largest |device - oracle| of test_feature_pass_vs_oracle_and_inference_untouched, fp32 mode, measured on the MI355X (absolute values;
# max|x| of the two references is 6.43 and 1.57): proposal level 3.218e-06, image level 7.997e-07
ORACLE_MEASURED_PROP = 3.218e-06
ORACLE_MEASURED_IMG = 7.997e-07


@pytest.fixture(scope="module", autouse=True)
def oracle_lib():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")], stdout=subprocess.DEVNULL)


def _f64(t):
    return t.detach().float().cpu().double().numpy() if t.dtype == torch.bfloat16 else t.detach().cpu().double().numpy()


# ------------------------------------------------------------------------------------------------ 1. pool_rows
@pytest.mark.parametrize("shape", [(1, 1, 8), (3, 49, 256), (2, 77, 256), (5, 273, 256), (1, 4096, 8)])
@pytest.mark.parametrize("mode", ["avg", "max"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_pool_rows_vs_fp64_of_the_same_operands(dtype, mode, shape):
    from aldi_amd import ops
    rows, S, C = shape
    g = torch.Generator().manual_seed(rows * 1000 + S)
    x = (torch.randn(rows, S, C, generator=g) * 3.0 + 0.5).to(dtype).to(DEV)
    out = torch.full((rows + 3, C), -7.0, dtype=torch.float32, device=DEV)
    ops.pool_rows(x, out, mode, row_off=2)                                       # a non-zero row offset, sentinel rows around it
    xd = _f64(x)
    ref = xd.mean(axis=1) if mode == "avg" else xd.max(axis=1)
    got = out.cpu().double().numpy()
    err = np.abs(got[2:2 + rows] - ref).max()
    tol = S * U32 * np.abs(xd).max() if mode == "avg" else 0.0
    print(f"pool_rows {dtype} {mode} {shape}: err {err:.3e} tol {tol:.3e}")
    assert err <= tol
    assert (got[:2] == -7.0).all() and (got[2 + rows:] == -7.0).all()


@pytest.mark.parametrize("mode", ["avg", "max"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_pool_rows_counted_compacts_in_order_without_touching_the_rest(dtype, mode):
    from aldi_amd import ops
    N, P, S, C = 3, 5, 49, 256
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, P, S, C, generator=g).to(dtype).to(DEV)
    count = torch.tensor([5, 0, 2], dtype=torch.int32, device=DEV)
    out = torch.full((N * P, C), 123.25, dtype=torch.float32, device=DEV)
    total = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    ops.pool_rows_counted(x, count, out, total, mode)
    assert int(total) == 7
    xd = _f64(x)
    valid = np.concatenate([xd[0, :5], xd[2, :2]])
    ref = valid.mean(axis=1) if mode == "avg" else valid.max(axis=1)
    got = out.cpu().double().numpy()
    tol = S * U32 * np.abs(xd).max() if mode == "avg" else 0.0
    assert np.abs(got[:7] - ref).max() <= tol
    assert (out[7:].cpu() == 123.25).all()                                       # sentinel rows bit-unchanged
    out2 = torch.full((N * P + 4, C), 123.25, dtype=torch.float32, device=DEV)   # and with a row offset
    ops.pool_rows_counted(x, count, out2, total, mode, row_off=4)
    assert torch.equal(out2[4:11], out[:7]) and (out2[:4].cpu() == 123.25).all() and (out2[11:].cpu() == 123.25).all()


# ------------------------------------------------------------------------------------------------ 2. moments_accum
def _acc(C):
    return (torch.zeros(C, dtype=torch.float64, device=DEV), torch.zeros(C, C, dtype=torch.float64, device=DEV),
            torch.zeros(1, dtype=torch.float64, device=DEV))


@pytest.mark.parametrize("C", [8, 256])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000, 4097])
def test_moments_accum_bounds_reproducibility_and_device_count(n, C):
    from aldi_amd import ops
    g = torch.Generator().manual_seed(n * 7 + C)
    X = (torch.randn(n, C, generator=g) + 0.5).to(DEV)
    ws = ops.moments_workspace(C, DEV)
    s1, g1, c1 = _acc(C)
    ops.moments_accum(X, s1, g1, c1, ws)
    Xd = X.cpu().double().numpy()
    Gref, Sref = Xd.T @ Xd, Xd.sum(axis=0)
    Gtol, Stol = n * U64 * (np.abs(Xd).T @ np.abs(Xd)), n * U64 * np.abs(Xd).sum(axis=0)
    dG, dS = np.abs(g1.cpu().numpy() - Gref), np.abs(s1.cpu().numpy() - Sref)
    print(f"moments n={n} C={C}: max dG {dG.max() if n else 0:.3e} (bound {Gtol.max() if n else 0:.3e}), max dS {dS.max() if n else 0:.3e}")
    assert (dG <= Gtol).all() and (dS <= Stol).all() and float(c1) == n
    assert torch.equal(g1, g1.T)
    # a second run from zeroed accumulators: the same bits
    s2, g2, c2 = _acc(C)
    ops.moments_accum(X, s2, g2, c2, ws)
    assert torch.equal(s1, s2) and torch.equal(g1, g2) and torch.equal(c1, c2)
    # n as a device word, X holding more rows than that: equals the host-n result
    s3, g3, c3 = _acc(C)
    Xpad = torch.cat([X, torch.full((37, C), 1e30, device=DEV)])
    ops.moments_accum(Xpad, s3, g3, c3, ws, n_dev=torch.tensor([n], dtype=torch.int32, device=DEV))
    assert torch.equal(s1, s3) and torch.equal(g1, g3) and torch.equal(c1, c3)
    # two calls on the halves agree with the call on the whole within the same bound
    s4, g4, c4 = _acc(C)
    h = n // 2
    ops.moments_accum(X[:h].contiguous(), s4, g4, c4, ws)
    ops.moments_accum(X[h:].contiguous(), s4, g4, c4, ws)
    assert (np.abs(g4.cpu().numpy() - Gref) <= Gtol).all() and (np.abs(s4.cpu().numpy() - Sref) <= Stol).all() and float(c4) == n
    # n = 0 (host and device form) leaves non-zero accumulators bit-unchanged
    s5, g5, c5 = s4.clone(), g4.clone(), c4.clone()
    g5[0, 0] = -0.0
    keep = (s5.clone(), g5.clone(), c5.clone())
    ops.moments_accum(X[:0].contiguous(), s5, g5, c5, ws)
    ops.moments_accum(Xpad, s5, g5, c5, ws, n_dev=torch.zeros(1, dtype=torch.int32, device=DEV))
    for a, b in zip(keep, (s5, g5, c5)):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))


# ------------------------------------------------------------------------------------------------ 3. project2
@pytest.mark.parametrize("n", [1, 65, 1000])
def test_project2_vs_fp64(n):
    from aldi_amd import ops
    C = 256
    g = torch.Generator().manual_seed(n)
    X = (torch.randn(n, C, generator=g) * 2.0 + 1.0).to(DEV)
    mean = torch.randn(C, generator=g, dtype=torch.float64).to(DEV)
    comp = torch.linalg.qr(torch.randn(C, 2, generator=g, dtype=torch.float64))[0].T.contiguous().to(DEV)
    Y = ops.project2(X, mean, comp)
    ref = (X.cpu().double().numpy() - mean.cpu().numpy()) @ comp.cpu().numpy().T
    err = np.abs(Y.cpu().double().numpy() - ref).max()
    print(f"project2 n={n}: err {err:.3e} bound {1e-6 * np.abs(ref).max():.3e}")
    assert Y.shape == (n, 2) and Y.dtype == torch.float32 and err <= 1e-6 * np.abs(ref).max()


# ------------------------------------------------------------------------------------------------ 4. the PCA chain on the device
@pytest.fixture(scope="module")
def chain():
    """the planted data set through moments_accum in three uneven chunks, pca_from_moments, project2"""
    from test_featurespace_cpu import planted
    from aldi_amd import ops
    from aldi_amd.featurespace import pca_from_moments
    X = torch.from_numpy(planted()).float().to(DEV)                              # what the device holds; the references see the same fp32 values
    xd = X.cpu().double().numpy()
    n, C = X.shape
    ws = ops.moments_workspace(C, DEV)
    s, g, c = _acc(C)
    for lo, hi in ((0, 77), (77, 1301), (1301, n)):
        ops.moments_accum(X[lo:hi].contiguous(), s, g, c, ws)
    res = pca_from_moments(s.cpu().numpy(), g.cpu().numpy(), float(c))
    Y = ops.project2(X, torch.from_numpy(res["mean"]).to(DEV), torch.from_numpy(res["components"]).to(DEV)).cpu().double().numpy()
    return xd, res, Y


def test_pca_chain_on_the_device_matches_numpy_svd(chain):
    from test_featurespace_cpu import svd_pca
    xd, res, Y = chain
    comp, evr, mean = svd_pca(xd)
    errs = {"components": np.abs(res["components"] - comp).max(), "evr": np.abs(res["explained_variance_ratio"] - evr).max(),
            "mean": np.abs(res["mean"] - mean).max()}
    print("device moments -> pca vs numpy svd:", errs)
    assert max(errs.values()) <= 1e-8, errs
    yref = (xd - mean) @ comp.T
    assert np.abs(Y - yref).max() <= 1e-6 * np.abs(yref).max()


def test_pca_chain_on_the_device_matches_sklearn(chain):
    skd = pytest.importorskip("sklearn.decomposition")
    xd, res, Y = chain
    ref = skd.PCA(2, svd_solver="full").fit(xd)
    assert np.abs(res["components"] - ref.components_).max() <= 1e-8
    assert np.abs(res["explained_variance_ratio"] - ref.explained_variance_ratio_).max() <= 1e-8
    yref = ref.transform(xd)
    assert np.abs(Y - yref).max() <= 1e-6 * np.abs(yref).max()


# ------------------------------------------------------------------------------------------------ 5. feature_pass
def _engine(dtype):
    from aldi_amd import synthetic as syn
    from aldi_amd.arch import ParamLayout
    from aldi_amd.engine import RCNN, Weights
    sd = syn.init_state_dict(K, seed=1)
    w = Weights(ParamLayout(K), torch.device(DEV), dtype, trainable=True)
    w.load_state_dict(sd)
    return sd, RCNN(w, K)


def _images():
    from aldi_amd import synthetic as syn
    g = torch.Generator().manual_seed(21)
    return [syn.make_image(160, 256, 6, K, g)[0], syn.make_image(192, 224, 9, K, g)[0]]      # canvas 192 x 256: both images padded


def _own_reference(m, images):
    """the engine's own intermediates, issued separately: p6 of a `trunk` call and RoIAlign on the proposals' rois"""
    from aldi_amd import ops
    from aldi_amd.arch import FPN_C, POOL
    st, sizes, hw = m.stage_images(images)
    c = m.trunk(st, sizes, save=False)
    m.rpn_head(c, save=False)
    N = st.shape[0]
    _, geom, anchors = m.geometry(st.shape[2], st.shape[3])
    props, _, pcount = m.proposals(c, geom, anchors, hw, N, training=False)
    P = props.shape[1]
    rois = torch.empty((N * P, 5), dtype=torch.float32, device=DEV)
    ops.rois_from_proposals(props, pcount, P, N, rois)
    pooled = torch.empty((N * P, POOL, POOL, FPN_C), dtype=m.dtype, device=DEV)
    ops.roialign(m.roi_feats(c), rois, N * P, POOL, pooled, backward=False)
    cnt = pcount.tolist()
    pd = _f64(pooled).reshape(N, P, POOL * POOL, FPN_C)
    return _f64(c.P[4]), np.concatenate([pd[i, :k] for i, k in enumerate(cnt)]), cnt, props.cpu()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("pooling", ["avg", "max"])
def test_feature_pass_equals_pooled_intermediates(dtype, pooling):
    _, m = _engine(dtype)
    images = _images()
    img, prop, total = m.feature_pass(images, pooling)
    p6, bins, cnt, _ = _own_reference(m, images)
    assert int(m.err) == 0 and int(total) == sum(cnt) and sum(cnt) > 0
    assert img.shape == (2, 256) and prop.shape[1] == 256 and img.dtype == prop.dtype == torch.float32
    p6 = p6.reshape(2, -1, 256)
    red = (lambda a: a.mean(axis=1)) if pooling == "avg" else (lambda a: a.max(axis=1))
    tol_img = p6.shape[1] * U32 * np.abs(p6).max() if pooling == "avg" else 0.0
    tol_prop = 49 * U32 * np.abs(bins).max() if pooling == "avg" else 0.0
    e_img = np.abs(img.cpu().double().numpy() - red(p6)).max()
    e_prop = np.abs(prop[: sum(cnt)].cpu().double().numpy() - red(bins)).max()
    print(f"feature_pass {dtype} {pooling}: rows {cnt}, img err {e_img:.3e} (tol {tol_img:.3e}), prop err {e_prop:.3e} (tol {tol_prop:.3e})")
    assert e_img <= tol_img and e_prop <= tol_prop


def test_feature_pass_vs_oracle_and_inference_untouched():
    from oracle import d2_rcnn as d2
    sd, m = _engine(torch.float32)
    images = _images()
    before = m.inference(images, 2.0).det
    img, prop, total = m.feature_pass(images)
    after = m.inference(images, 2.0).det
    for k in ("boxes", "scores", "classes", "count"):                            # no workspace shared destructively
        assert torch.equal(before[k], after[k]), k
    _, _, cnt, props = _own_reference(m, images)
    cfg = d2.make_cfg(num_classes=K)
    with torch.no_grad():
        x, _ = d2.preprocess(cfg, images)
        feats = d2.resnet_fpn(cfg, sd, x)
        pooled = d2.roi_pool(cfg, [feats[k] for k in ("p2", "p3", "p4", "p5")], [props[i, :n] for i, n in enumerate(cnt)])
    ref_prop = pooled.double().mean(dim=(2, 3)).numpy()
    ref_img = feats["p6"].double().mean(dim=(2, 3)).numpy()
    d_prop, x_prop = np.abs(prop[: sum(cnt)].cpu().double().numpy() - ref_prop).max(), np.abs(ref_prop).max()
    d_img, x_img = np.abs(img.cpu().double().numpy() - ref_img).max(), np.abs(ref_img).max()
    b_prop, b_img = min(4 * ORACLE_MEASURED_PROP, 1e-3 * x_prop), min(4 * ORACLE_MEASURED_IMG, 1e-3 * x_img)
    print(f"feature_pass vs oracle: prop max|d| {d_prop:.3e} (max|x| {x_prop:.3e}, bound {b_prop:.3e}), "
          f"img max|d| {d_img:.3e} (max|x| {x_img:.3e}, bound {b_img:.3e})")
    assert d_prop <= b_prop and d_img <= b_img


# ------------------------------------------------------------------------------------------------ 6. collector and tool
CONFIG = os.path.join(ROOT, "configs", "cityscapes", "ALDI-Best-Cityscapes.yaml")
SMALL = ["SYNTHETIC.HEIGHT", H, "SYNTHETIC.WIDTH", W, "SYNTHETIC.VAL_IMAGES", 4, "SEED", 1]


def test_collector_end_to_end():
    from aldi_amd.config import add_aldi_config, get_cfg
    from aldi_amd.featurespace import FeatureSpaceCollector
    from aldi_amd.trainer import ALDITrainer
    cfg = get_cfg()
    add_aldi_config(cfg)
    cfg.merge_from_file(CONFIG)
    cfg.merge_from_list(SMALL)
    model = ALDITrainer.build_model(cfg)
    names = ("source_val", "target_val")
    col = FeatureSpaceCollector(model)
    for name in names:
        col.collect(name, ALDITrainer.build_test_loader(cfg, name))
    lean = FeatureSpaceCollector(model, keep_features=False)
    for name in names:
        lean.collect(name, ALDITrainer.build_test_loader(cfg, name))
    for level in ("image", "proposal"):
        res = col.pca(level)
        evr = res["explained_variance_ratio"]
        assert res["components"].shape == (2, 256) and res["mean"].shape == (256,)
        assert all(0.0 < v <= 1.0 for v in evr) and evr.sum() <= 1.0, evr
        total = 0
        for name in names:
            n = col.count(name, level)
            total += n
            assert n == (4 if level == "image" else n) and n > 0
            xy = res["coords"][name]
            assert xy.shape == (n, 2) and xy.dtype == np.float32
            ref = (col.features(name, level).cpu().double().numpy() - res["mean"]) @ res["components"].T
            assert np.abs(xy - ref).max() <= 1e-6 * np.abs(ref).max()
        assert res["count"] == total
        a, b = col.moments(level), lean.moments(level)
        assert "coords" not in lean.pca(level)
        assert a["count"] == b["count"] and np.array_equal(a["sum"], b["sum"]) and np.array_equal(a["gram"], b["gram"])
        assert np.array_equal(a["mean"], b["mean"]) and np.array_equal(a["cov"], b["cov"])
        assert lean.count(names[1], level) == col.count(names[1], level)


@pytest.fixture(scope="module")
def tool_output(tmp_path_factory):
    import importlib.util
    out = str(tmp_path_factory.mktemp("featurespace"))
    spec = importlib.util.spec_from_file_location("visualize_featurespace", os.path.join(ROOT, "tools", "visualize_featurespace.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tool.main(["--config-file", CONFIG, "OUTPUT_DIR", out] + [str(v) for v in SMALL])
    return tool, out


def test_tool_writes_npz(tool_output):
    tool, out = tool_output
    z = np.load(os.path.join(out, "featurespace.npz"))
    assert list(z["datasets"]) == list(tool.SYNTHETIC_NAMES)
    for level, rows in (("image", 4), ("proposal", None)):
        assert z[f"{level}_components"].shape == (2, 256) and z[f"{level}_explained_variance_ratio"].shape == (2,)
        for i in range(2):
            xy = z[f"{level}_coords_{i}"]
            assert xy.ndim == 2 and xy.shape[1] == 2 and (rows is None or xy.shape[0] == rows) and np.isfinite(xy).all()


def test_tool_writes_plots_when_matplotlib_imports(tool_output):
    pytest.importorskip("matplotlib")
    _, out = tool_output
    for level in ("image", "proposal"):
        assert os.path.getsize(os.path.join(out, f"feature_vis_{level}_pca.png")) > 0


# ------------------------------------------------------------------------------------------------ 7. other engines are rejected
def test_other_engines_are_rejected_by_name():
    from aldi_amd.config import CfgNode, add_aldi_config, get_cfg
    from aldi_amd.featurespace import FeatureSpaceCollector
    from aldi_amd.model import build_aldi
    cfg = get_cfg()
    add_aldi_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "cityscapes", "ALDI-VitDetB-Cityscapes.yaml"))
    cfg.merge_from_list(["SOLVER.IMS_PER_BATCH", 2, "SEED", 1, "SYNTHETIC.HEIGHT", 128, "SYNTHETIC.WIDTH", 160])
    cfg.SYNTHETIC.VIT = CfgNode(dict(embed=128, depth=4, heads=2, window=7, global_blocks=(1, 3), pretrain_grid=4, rel_input=10))
    model = build_aldi(cfg)
    with pytest.raises(ValueError, match="only the R50-FPN engine"):
        FeatureSpaceCollector(model)
    with pytest.raises(ValueError, match="only the R50-FPN engine"):
        model.engine.feature_pass([torch.zeros(3, 128, 160, dtype=torch.uint8)])

"""The autograd path of every flat-parameter family (flat._FlatFunction): the activations a backward reads live in one workspace per
batch size, so a second forward of that size between a forward and its backward must raise (params.ForwardTape) instead of giving
wrong gradients; a fresh forward + backward then gives the fused step's gradients, at the tolerance each family's own autograd-vs-fused
test asserts."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _stgnn():
    from gnn_rul_benchmarking_amd.stgnn import STGNN_model
    torch.manual_seed(1)
    cfg = dict(patch_size=10, num_patch=5, num_nodes=20, hidden_dim=64, K=3, top_k=10)
    x, y = torch.rand(7, 20, 50, device=DEV) * 2 - 1, torch.rand(7, 1, device=DEV)
    sd = {k: v.clone() for k, v in STGNN_model(**cfg).state_dict().items()}

    def build():
        m = STGNN_model(**cfg)
        m.load_state_dict(sd)
        return m.to(DEV)
    return build, x, y


def _stgcn():
    from gnn_rul_benchmarking_amd import _lib
    from gnn_rul_benchmarking_amd.stgcn import ST_GCN_model
    torch.manual_seed(1)
    x, y = torch.rand(16, 14, 30, device=DEV), torch.rand(16, 1, device=DEV)
    sd = {k: v.clone() for k, v in ST_GCN_model(14, 30, dropout=0.2).state_dict().items()}

    def build():
        m = ST_GCN_model(14, 30, dropout=0.2)
        m.load_state_dict(sd)
        m._seed = 5                                  # one dropout stream for both models
        m.step_path = _lib.STEP_CHAIN                # the fused step on the fp32 phases, the arithmetic of the forward / backward entries
        return m.to(DEV)
    return build, x, y


def _golden(module, case, build_args=lambda T, z, rest: rest, **kw):
    """(model factory, x, y) of a family's golden case, built by that family's own GPU-test helpers."""
    T = __import__(module)
    z, *rest = T.load_case(case)
    args = build_args(T, z, rest)
    x, y = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["y"]).to(DEV)
    return (lambda: T.build_model(*args, **kw)), x, y


def _sd(z):
    return {k[3:]: z[k] for k in z.files if k.startswith("sd:")}


# family -> (inputs, gradient tolerance of the family's own autograd-vs-fused test; None: bit-exact)
FAMILIES = {
    "ST_GCN": (_stgcn, (5e-4, 1e-6)),
    "STGNN": (_stgnn, (1e-4, 1e-7)),
    "STNet": (lambda: _golden("test_stnet_gpu", "stnet_phm_c3like_7x32_bs4"), None),
    "SAGCN": (lambda: _golden("test_sagcn_gpu", "sagcn_phm_c2like_9x20_bs4"), None),
    "RGCNU": (lambda: _golden("test_rgcnu_gpu", "rgcnu_cmapss_14x50_bs7", dropout=0.5), None),
    "STAGNN": (lambda: _golden("test_stagnn_gpu", "stagnn_cmapss_fd002_h16_bs7"), None),
    "ST_Conv": (lambda: _golden("test_stconv_gpu", "stconv_small_6x11_bs9", lambda T, z, rest: [T.cfg_of(z), _sd(z)]), (1e-5, 1e-8)),
    "STMSGCN": (lambda: _golden("test_stmsgcn_gpu", "stmsgcn_phm2_9x20_bs4"), (1e-6, 1e-9)),
    "FC_STGNN": (lambda: _golden("test_fcstgnn_gpu", "fcstgnn_fd004_bs6", lambda T, z, rest: [rest[0], _sd(z)], dropout=0.1), (1e-4, 1e-7)),
    "ASTGCNN": (lambda: _golden("test_astgcnn_gpu", "astgcnn_small_5x12_bs9", lambda T, z, rest: [T.cfg_of(z), _sd(z)]), (1e-5, 1e-8)),
}


def _loss(family, m, x, y):
    """The loss ``fused_mse_step`` minimises, through autograd: STNet's adds its reconstruction term."""
    if family == "STNet":
        pred, recon = m(x, train=True)
        return torch.nn.functional.mse_loss(pred, y) + recon
    return torch.nn.functional.mse_loss(m(x), y)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_backward_after_a_second_forward_raises_and_a_fresh_one_matches_the_fused_step(family):
    inputs, tol = FAMILIES[family]
    build, x, y = inputs()
    m = build().train()
    loss1 = _loss(family, m, x, y)
    with torch.no_grad():
        m(x * 0.5)                                   # e.g. an evaluation inside the step
    with pytest.raises(RuntimeError, match="overwritten"):
        loss1.backward()
    _loss(family, m, x, y).backward()
    auto = torch.cat([(t.grad if t.grad is not None else torch.zeros_like(t)).reshape(-1) for t in m._named()])
    m2 = build().train()
    if hasattr(m, "_step"):                          # dropout masks are drawn per step: the fused step must draw the forward's
        m2._step = m._step - 1
    m2.fused_mse_step(x, y)
    fused = m2._grad_flat[:m2.num_live]
    assert float(fused.abs().max()) > 0
    if tol is None:
        assert torch.equal(auto, fused)
    else:
        assert torch.allclose(auto, fused, rtol=tol[0], atol=tol[1])

"""The class-token tail: VisionTransformer's head reads token 0 only, so its last block computes that row alone
(TransformerBlock.run_cls: q layers, single-query attention, residual, LN2 and feed-forward on the B class rows; k and v on all
rows).  Checked on a width the fused small feed-forward does not cover (the small geometries keep their own path), N = 17, B = 3:
against oracle.vit_forward in float64 at the project's 1e-4, and against the same tree with KANVIT_NO_CLS_TAIL=1 -- every row
computed, as before -- at 1e-5 of each array's maximum (not bitwise: the GEMMs and the attention run other shapes)."""
import collections
import contextlib
import functools
import os
import re

import pytest
import torch

from oracle import kan_oracle as ko
from tests._util import close, kernel_name, max_err, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4
TYPES = ["vanilla", "flash-attn", "efficientkan", "sine", "fourier", "cheby", "fast", "sine,fourier"]
HEADS, PATCHES, B = 2, 4, 3


@contextlib.contextmanager
def _every_row():
    """The path before the class-token tail: the last block computes every row."""
    from kanvit import _lib
    os.environ["KANVIT_NO_CLS_TAIL"] = "1"
    try:
        assert _lib.reload_config().endswith("py_no_cls_tail=1")
        yield
    finally:
        del os.environ["KANVIT_NO_CLS_TAIL"]
        assert _lib.reload_config().endswith("py_no_cls_tail=0")


def _width():
    """The narrowest width from 128 up whose feed-forward the fused small kernel does not take: there the tail applies."""
    from kanvit.dense import ff_small_supported
    d = 128
    while ff_small_supported(d, 4 * d):
        d += 64
    return d


@functools.lru_cache(maxsize=None)
def _case(kind, n_blocks=2):
    """(model on the CPU, images, labels, oracle logits, oracle loss, oracle gradients) -- built once per type and shared."""
    from model import VisionTransformer
    torch.manual_seed(23)
    m = VisionTransformer((3, 32, 32), n_patches=PATCHES, n_blocks=n_blocks, d_hidden=_width(), n_heads=HEADS, out_d=10, type=kind)
    x = torch.randn(B, 3, 32, 32)
    labels = torch.tensor([3, 7, 1])
    sd = {k: (v.detach().double() if v.is_floating_point() else v) for k, v in m.state_dict().items()}
    params = {k: v.clone().requires_grad_(not ko.is_buffer_key(k) and v.is_floating_point()) for k, v in sd.items()}
    ref = ko.vit_forward(params, x.double(), PATCHES, HEADS, kind.split(",")[0])
    ref_loss = torch.nn.functional.cross_entropy(ref, labels)
    ref_loss.backward()
    return m, x, labels, ref.detach(), float(ref_loss), {k: v.grad for k, v in params.items() if v.grad is not None}


def _train_pass(kind, n_blocks=2, autocast=False):
    """logits, loss and every parameter gradient of one forward + backward on the GPU (a fresh copy of the case's model)."""
    import copy
    m0, x, labels, *_ = _case(kind, n_blocks)
    m = copy.deepcopy(m0).to(DEV)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        logits = m(x.to(DEV))
        loss = torch.nn.functional.cross_entropy(logits.float(), labels.to(DEV))
    loss.backward()
    grads = {k: (None if p.grad is None else p.grad.detach().cpu()) for k, p in m.named_parameters() if p.requires_grad}
    return logits.detach().float().cpu(), float(loss), grads


def test_the_width_under_test_takes_the_tail():
    from kanvit.dense import ff_small_supported
    d = _width()
    assert not ff_small_supported(d, 4 * d)
    assert d == 128 or ff_small_supported(128, 512)


# every type with two blocks (the last block receives a pending feed-forward output), three of them with one (it does not)
MODELS = [(k, 2) for k in TYPES] + [("cheby", 1), ("vanilla", 1), ("fast", 1)]


@pytest.mark.parametrize("kind,n_blocks", MODELS)
def test_cls_tail_against_the_oracle_and_the_every_row_path(kind, n_blocks):
    _, _, _, ref, ref_loss, ref_grads = _case(kind, n_blocks)
    logits, loss, grads = _train_pass(kind, n_blocks)
    with _every_row():
        logits0, loss0, grads0 = _train_pass(kind, n_blocks)
    print(f"{kind} x{n_blocks}: logits vs oracle {max_err(logits, ref):.2e}, loss {abs(loss - ref_loss):.2e}, vs every-row path {rel_err(logits, logits0):.2e}")
    assert max_err(logits, ref) < TOL
    assert abs(loss - ref_loss) < TOL
    assert set(grads) == set(grads0)
    for k in grads:
        g = ref_grads[k]
        assert grads[k] is not None and grads0[k] is not None, k
        # 1e-4 of the largest entry; the absolute term is for tensors that are mathematically zero (the key biases: softmax is
        # shift invariant), whose computed values are rounding noise on both sides
        assert close(grads[k], g, rtol=TOL, atol=2e-7), (kind, k, rel_err(grads[k], g, floor=1e-6))
    assert rel_err(logits, logits0) <= 1e-5
    assert abs(loss - loss0) <= 1e-5 * max(1.0, abs(loss0))
    for k in grads:
        assert rel_err(grads[k], grads0[k]) <= 1e-5, (kind, k, rel_err(grads[k], grads0[k]))


@pytest.mark.parametrize("kind", ["cheby", "efficientkan"])
def test_cls_tail_in_eval_mode_without_gradients(kind):
    import copy
    m0, x, _, ref, _, _ = _case(kind)
    m = copy.deepcopy(m0).to(DEV).eval()
    with torch.no_grad():
        logits = m(x.to(DEV)).cpu()
        with _every_row():
            logits0 = m(x.to(DEV)).cpu()
    assert not logits.requires_grad
    assert max_err(logits, ref) < TOL
    assert rel_err(logits, logits0) <= 1e-5


def test_regularised_forward_keeps_the_every_row_path():
    """return_regularization=True needs LN1's output for every layer of the block anyway: the switch changes nothing."""
    import copy
    m0, x, _, _, _, _ = _case("cheby")
    m = copy.deepcopy(m0).to(DEV)
    logits, reg = m(x.to(DEV), return_regularization=True)
    with _every_row():
        logits0, reg0 = m(x.to(DEV), return_regularization=True)
    assert torch.equal(logits, logits0) and torch.equal(reg, reg0)


def test_cls_tail_under_bf16_autocast():
    """Under bf16 autocast the q|k|v launch and the attention stay on the bf16 matrix cores for every row; LN2 and the feed-forward
    take the class rows.  Against the every-row path: bf16 GEMMs of another shape, so bf16-sized bounds, relative to the maximum."""
    logits, loss, grads = _train_pass("cheby", autocast=True)
    with _every_row():
        logits0, loss0, grads0 = _train_pass("cheby", autocast=True)
    print(f"bf16: logits {rel_err(logits, logits0):.2e}, worst gradient {max(rel_err(grads[k], grads0[k]) for k in grads):.2e}")
    assert rel_err(logits, logits0) <= 1e-3
    for k in grads:
        assert grads[k] is not None and grads0[k] is not None, k
        assert rel_err(grads[k], grads0[k]) <= 1e-2, (k, rel_err(grads[k], grads0[k]))


def _kernel_counts(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA], acc_events=True) as prof:
        fn()
        torch.cuda.synchronize()
    counts = collections.Counter(kernel_name(e.name) for e in prof.events() if e.device_type != torch.autograd.DeviceType.CPU)
    assert counts, "torch.profiler recorded no device kernel"
    return counts


def test_cls_tail_launches_the_single_query_kernels():
    def step():
        _train_pass("cheby")

    step()                                                                # module load, packing caches
    new = _kernel_counts(step)
    with _every_row():
        old = _kernel_counts(step)
    fwd = re.compile(r"attn(16|_small|_x)?_fwd")
    q1 = {n: c for n, c in new.items() if n.startswith("attn_q1")}
    assert sorted(q1) == ["attn_q1_bwd_kernel<4>", "attn_q1_fwd_kernel<4>"] and set(q1.values()) == {1}, q1
    assert not [n for n in old if n.startswith("attn_q1")]
    assert sum(c for n, c in new.items() if fwd.match(n)) == sum(c for n, c in old.items() if fwd.match(n)) - 1, (new, old)

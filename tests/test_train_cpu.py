"""CPU-only checks of the drop-in's host side: train.py's command line (the reference's flags verbatim, train.py:87-97),
the reporting helpers against output of the reference's own (tests/golden/metrics.npz, made by make_golden.py from
utils.py:13-47,79-94), the per-block type extension of BASELINE configs[4], and argument validation."""
import os

import numpy as np
import pytest
import torch

from tests._util import load_npz


def test_command_line_is_the_references():
    import train
    a = train.parse([])
    ref = dict(epochs=20, batch_size=128, learning_rate=0.001, model_type="vanilla", n_blocks=8, d_hidden=64, n_heads=8,
               log_dir="logs")                                                    # train.py:88-96 defaults
    for k, v in ref.items():
        assert getattr(a, k) == v, k
    assert a.device in ("cuda", "cpu")
    # the geometry train.py:19 hard-codes is the default of the added flags; the fast paths are opt-in
    assert (a.in_chans, a.image_size, a.n_patches, a.out_d) == (3, 32, 4, 100)
    assert a.amp == "off" and a.graph is False and a.dp is False
    b = train.parse(["--model-type", "cheby", "--amp", "bf16", "--graph", "--epochs", "1"])
    assert (b.model_type, b.amp, b.graph, b.epochs) == ("cheby", "bf16", True, 1)


def test_train_refuses_to_run_the_hot_path_on_the_cpu():
    import train
    with pytest.raises(SystemExit):
        train.main(train.parse(["--device", "cpu", "--synthetic", "--epochs", "1"]))


def test_complete_fills_a_hand_built_namespace_from_the_parser():
    """train.complete: a namespace built by hand reads like one from parse(); given values stay; a second call changes nothing; and
    every flag has a default to fill in."""
    import argparse
    import train
    by_hand = train.complete(argparse.Namespace(synthetic=True))
    assert vars(by_hand) == vars(train.parse(["--synthetic"]))
    before = dict(vars(by_hand))
    assert train.complete(by_hand) is by_hand and vars(by_hand) == before
    kept = train.complete(argparse.Namespace(weight_decay=0.1, rrc_scale=(0.5, 0.75)))
    assert kept.weight_decay == 0.1 and kept.rrc_scale == (0.5, 0.75) and kept.synthetic is False
    dests = {a.dest: a.default for a in train.build_parser()._actions if a.dest != "help"}       # -h stores nothing
    assert dests.keys() == vars(train.parse([])).keys() and len(dests) > 50
    assert all(default is not argparse.SUPPRESS for default in dests.values())


@pytest.mark.parametrize("argv, word", [
    (["--model-type", "efficientkan", "--grid-extend", "3:10", "--graph"], "--grid-extend is not combined with --graph"),
    (["--model-type", "cheby", "--grid-update-every", "2"], "--grid-update-every: model type 'cheby' has no KANLinear"),
    (["--model-type", "sine", "--prune", "3:0.5"], "--prune: model type\\(s\\) sine have no edge-activation statistic"),
    (["--device", "cpu"], "--device must be a cuda device")])
def test_what_only_a_run_refuses_passes_parse_and_stops_main_before_the_gpu(argv, word):
    import train
    args = train.parse(["--synthetic", "--device", "cuda", *argv])      # parse() takes it ...
    with pytest.raises(SystemExit, match=word):
        train.main(args)                                                # ... main() refuses it, with no GPU in sight


def test_save_metrics_is_byte_identical_to_the_reference(tmp_path):
    from utils import save_metrics
    fn = str(tmp_path / "logs" / "m.txt")
    save_metrics(fn, 20, "Train", 1.23456789, 0.5, 0.25, 0.125, 0.0625, 0)
    save_metrics(fn, 20, "Test", 4.60517, 0.01, 0.0123456, 0.99995, 0.5, 1)
    want = load_npz("metrics.npz")["save_metrics_text"].tobytes()
    assert open(fn, "rb").read() == want


def test_calculate_metrics_matches_the_reference():
    from utils import calculate_metrics
    m = load_npz("metrics.npz")
    got = calculate_metrics(m["cm.y_true"], m["cm.y_pred"], m["cm.proba"])
    assert np.allclose(got, m["cm.out"], rtol=0, atol=1e-12)


def test_mixed_block_types_keep_the_reference_layout_per_block():
    """BASELINE configs[4] (SineKAN + FourierKAN mixed blocks): block l of type 'a,b' has exactly the parameters of block l
    of the single-type model of its own type; the patch embedding follows the first entry."""
    from model import VisionTransformer, split_types
    assert split_types("sine") == ["sine"] and split_types("sine+fourier") == ["sine", "fourier"]
    geo = dict(chw=(1, 28, 28), n_patches=7, n_blocks=4, d_hidden=64, n_heads=2, out_d=10)
    mixed = VisionTransformer(**geo, type="sine,fourier")
    sine = VisionTransformer(**geo, type="sine")
    four = VisionTransformer(**geo, type="fourier")
    shapes = {k: tuple(v.shape) for k, v in mixed.state_dict().items()}
    want = {}
    for k, v in sine.state_dict().items():
        if not k.startswith("blocks.") or int(k.split(".")[1]) % 2 == 0:
            want[k] = tuple(v.shape)
    for k, v in four.state_dict().items():
        if k.startswith("blocks.") and int(k.split(".")[1]) % 2 == 1:
            want[k] = tuple(v.shape)
    assert shapes == want
    with pytest.raises(ValueError):
        VisionTransformer(**geo, type="sine,flash-attn")
    with pytest.raises(ValueError):
        VisionTransformer(**geo, type="")


def test_attention_shape_checks_happen_before_any_launch():
    """The self-attention binding (kanvit_attn_desc: ONE sequence length) refuses q / k / v of different shapes before any launch;
    FlashAttentionFunction routes q_len != k_len and masks to the general kernels (kanvit_attn_x_*), which -- like every kanvit
    op -- refuse CPU tensors instead of falling back, and refuses `causal` with k_len > q_len (utils.py:169,183: ill-defined)."""
    from utils import FlashAttentionFunction
    from kanvit import KanvitError, ops
    q = torch.randn(1, 2, 8, 16)
    for kv_len in (5, 12):
        k = torch.randn(1, 2, kv_len, 16)
        with pytest.raises(KanvitError):                                # CPU tensors: no fallback
            FlashAttentionFunction.apply(q, k, k, None, False, 512, 1024)
    with pytest.raises(NotImplementedError):
        FlashAttentionFunction.apply(q, torch.randn(1, 2, 12, 16), torch.randn(1, 2, 12, 16), None, True, 512, 1024)
    with pytest.raises(ValueError):                                     # v does not match k
        FlashAttentionFunction.apply(q, torch.randn(1, 2, 12, 16), torch.randn(1, 2, 11, 16), None, False, 512, 1024)
    with pytest.raises(KanvitError):
        ops._attn_desc(q, torch.randn(1, 2, 5, 16), q, q, False, 0.25)
    with pytest.raises(KanvitError):
        ops._attn_desc(q, q, torch.randn(1, 3, 8, 16), q, False, 0.25)


def test_bench_self_launches_its_ranks(tmp_path):
    """`python bench.py --gpus 2` invoked PLAINLY (no torch.distributed.run, no RANK): the parent spawns the two ranks as
    children before touching any GPU, relays rank 0's one JSON line and propagates the exit code.  The --rendezvous-only
    hook stops each rank after the process group is up (gloo here: no GPU in this container)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, KANVIT_DIST_BACKEND="gloo")
    env.pop("RANK", None), env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--rendezvous-only"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout                                  # ONE line on stdout, whatever the launcher printed
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["sum_of_ones"] == 2.0
    # a failing rank's exit code comes back through the parent (a backend that does not exist fails inside every CHILD)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--rendezvous-only"],
                       env=dict(env, KANVIT_DIST_BACKEND="no-such-backend"), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "launching" in r.stderr and not r.stdout.strip()


def test_bench_dump_outputs_are_float_fixed_and_bounded(tmp_path):
    """bench.py --dump-outputs: float .npy files under 64 MB in all, and the sampled positions of a model larger than the
    sample (ViT-S here) are the same from run to run, so two builds can be compared output for output."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from model import VisionTransformer
    wl = bench.WORKLOADS["vits16-224-cheby"]
    torch.manual_seed(0)
    m = VisionTransformer(wl["chw"], wl["n_patches"], wl["n_blocks"], wl["d"], wl["heads"], wl["out_d"], type=wl["type"])
    params = [p for p in m.parameters() if p.requires_grad]
    n = sum(p.numel() for p in params)
    assert n > bench.DUMP_SAMPLE
    for i, p in enumerate(params):
        p.grad = torch.full_like(p, float(i))                     # the gradient names the parameter it belongs to
    logits = torch.randn(wl["batch"], wl["out_d"])
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), m, logits, torch.tensor(1.5))
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["grads.npy", "logits.npy", "loss.npy", "params.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    for k, a in got.items():
        assert np.array_equal(a, np.load(tmp_path / "b" / f"{k}.npy"))
    assert np.array_equal(got["logits"], logits.numpy()) and got["loss"].tolist() == [1.5]
    assert got["grads"].shape == got["params"].shape == (bench.DUMP_SAMPLE,)
    # sorted positions over the flattened parameters: the parameter indices they fall in never decrease, and span the model
    g = got["grads"]
    assert np.all(np.diff(g) >= 0) and g[0] == 0 and g[-1] == len(params) - 1
    flat = torch.cat([p.detach().reshape(-1) for p in params]).numpy()
    assert np.isin(got["params"], flat).all()

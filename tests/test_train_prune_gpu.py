"""train.py --prune on the GPU: six steps of a tiny model with `--prune 3:0.5`, for stock Adam, for kanvit-adamw with decay, clipping,
warm-up and EMA, and under --graph.  After the run every masked run of the parameters, the moments and the EMA is exactly 0; the
eager runs equal, bitwise, the same loop with the masking restated in stock torch (in-place grad[~mask] = 0 before the step, the
state zeroed at step 3)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
GEOMETRY = ["--n-blocks", "1", "--d-hidden", "16", "--n-heads", "2", "--image-size", "8", "--n-patches", "2", "--out-d", "10", "--epochs", "1",
            "--synthetic", "--no-step-metrics"]
RECIPE = ["--optimizer", "kanvit-adamw", "--weight-decay", "0.05", "--clip-grad-norm", "0.5", "--warmup-steps", "2", "--ema-decay", "0.9"]
STEPS, PRUNE_STEP = 6, 3
_RUNS = {}


def _batches():
    g = torch.Generator().manual_seed(7)
    return [(torch.randn(8, 3, 8, 8, generator=g), torch.randint(0, 10, (8,), generator=g)) for _ in range(STEPS)]


def _init(kind):
    """One initial state per model type: KANLinear's least-squares initialisation is not bitwise reproducible."""
    if ("init", kind) not in _RUNS:
        from model import VisionTransformer
        torch.manual_seed(9)
        _RUNS["init", kind] = {k: v.clone() for k, v in VisionTransformer((3, 8, 8), 2, 1, 16, 2, 10, type=kind).state_dict().items()}
    return _RUNS["init", kind]


def _args(kind, extra, tmp_path, prune=True):
    import train
    return train.parse(["--model-type", kind, *GEOMETRY, *(["--prune", f"{PRUNE_STEP}:0.5"] if prune else []), *extra,
                        "--log-dir", str(tmp_path / f"logs{len(_RUNS)}")])


def _train(kind, extra, tmp_path):
    import train
    key = (kind, tuple(extra))
    if key not in _RUNS:
        _RUNS[key] = train.main(_args(kind, extra, tmp_path), batches=_batches(), init_state=_init(kind))
    return _RUNS[key]


def _state(optimizer, p):
    """The optimizer's per-parameter state tensors: moments (and EMA) of either optimizer."""
    from kanvit.optim import KanvitAdamW
    if isinstance(optimizer, KanvitAdamW):
        return list(optimizer.moments(p)) + ([optimizer.ema(p)] if "ema" in optimizer.flat else [])
    return [optimizer.state[p]["exp_avg"], optimizer.state[p]["exp_avg_sq"]]


def _dead(t, mask, run):
    """The masked runs of t, seen as rows of `run`."""
    return t.detach().reshape(mask.numel(), run)[mask.reshape(-1) == 0]


def _restated(kind, extra, tmp_path):
    """train.py's eager step without --prune's machinery: the masking in stock torch."""
    import train
    from kanvit import tuned
    from kanvit.optim import KanvitAdamW
    from model import VisionTransformer
    args = _args(kind, extra, tmp_path, prune=False)
    torch.manual_seed(args.seed)
    model = VisionTransformer((3, 8, 8), n_patches=2, n_blocks=1, d_hidden=16, n_heads=2, out_d=10, type=kind)
    model.load_state_dict(_init(kind))
    model = model.to(DEV)
    tuned.enable_tuned_gemms()
    if args.optimizer == "adam":
        optimizer = torch.optim.Adam(model.parameters(), lr=args.learning_rate, fused=True, capturable=False)
    else:
        optimizer = KanvitAdamW(model.parameters(), lr=args.learning_rate, weight_decay=args.weight_decay, max_grad_norm=args.clip_grad_norm,
                                ema_decay=args.ema_decay, total_steps=STEPS, warmup_steps=args.warmup_steps, schedule=args.lr_schedule,
                                min_lr=args.min_lr)
    criterion = torch.nn.CrossEntropyLoss()
    triples = model.edge_masked()
    model.train()
    losses = []
    for n, (x, y) in enumerate(_batches(), start=1):
        x, y = x.to(DEV), y.to(DEV)
        if n == PRUNE_STEP:
            model.prune_edges(x, fraction=0.5)
            with torch.no_grad():
                for p, mask, run in triples:
                    for t in _state(optimizer, p):
                        t.view(mask.numel(), run)[mask.reshape(-1) == 0] = 0.0
        loss = criterion(model(x).float(), y)
        optimizer.zero_grad()
        loss.backward()
        with torch.no_grad():
            for p, mask, run in triples:
                p.grad.view(mask.numel(), run)[mask.reshape(-1) == 0] = 0.0
        optimizer.step()
        losses.append(float(loss.detach()))
    return model, optimizer, losses


def _check_pruned_state(run, kind):
    model, optimizer = run["model"], run["optimizer"]
    triples = model.edge_masked()
    assert triples
    kept = total = 0
    for p, mask, run_ in triples:
        for t in [p] + _state(optimizer, p):
            dead = _dead(t, mask, run_)
            assert dead.numel() > 0 and bool((dead.view(torch.int32) == 0).all()), (tuple(p.shape), run_)     # +0.0 exactly
        alive = p.detach().reshape(mask.numel(), run_)[mask.reshape(-1) == 1]
        assert bool((alive != 0).any(dim=1).all())                    # and the kept edges are alive
    for mask in {id(m): m for _, m, _ in triples}.values():
        E = mask.numel()
        assert int(mask.sum()) == E - int(0.5 * E)
        kept, total = kept + int(mask.sum()), total + E
    assert total == 48 * 16 + 6 * 64
    assert run["edges"] == [(kept, total)]                            # logged once per epoch
    assert len(run["losses"]) == STEPS and all(v == v and abs(v) != float("inf") for v in run["losses"])


@pytest.mark.parametrize("kind,extra", [("cheby", []), ("efficientkan", []), ("cheby", RECIPE), ("fast", RECIPE)],
                         ids=["cheby-adam", "efficientkan-adam", "cheby-adamw", "fast-adamw"])
def test_eager_run_holds_pruned_edges_at_zero_and_equals_the_torch_restatement(kind, extra, tmp_path):
    run = _train(kind, extra, tmp_path)
    _check_pruned_state(run, kind)
    model, optimizer, losses = _restated(kind, extra, tmp_path)
    print("losses:", run["losses"], losses)
    assert run["losses"] == losses
    mine, theirs = dict(run["model"].named_parameters()), dict(model.named_parameters())
    assert list(mine) == list(theirs)
    for name in mine:
        assert torch.equal(mine[name].detach().view(torch.int32), theirs[name].detach().view(torch.int32)), name
        if mine[name].requires_grad:                                  # FastKAN's frozen rbf.grid has no optimizer state
            for a, b in zip(_state(run["optimizer"], mine[name]), _state(optimizer, theirs[name])):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    for (_, a, _), (_, b, _) in zip(run["model"].edge_masked(), model.edge_masked()):
        assert torch.equal(a, b)
    if extra:
        # the clip norm is the norm of the gradients that are used: the parameters still hold the last step's masked gradients
        for p, mask, run_ in run["model"].edge_masked():
            assert bool((_dead(p.grad, mask, run_) == 0).all())
        sumsq = sum(float(p.grad.double().pow(2).sum()) for p in run["model"].parameters() if p.grad is not None)
        norm = sumsq ** 0.5
        print("grad norm:", run["grad_norm"], norm)
        assert abs(run["grad_norm"] - norm) <= 1e-6 * norm


def test_pruning_changes_nothing_before_its_step(tmp_path):
    import train
    run = _train("cheby", [], tmp_path)
    plain = train.main(_args("cheby", [], tmp_path, prune=False), batches=_batches(), init_state=_init("cheby"))
    assert run["losses"][:PRUNE_STEP - 1] == plain["losses"][:PRUNE_STEP - 1] and run["losses"] != plain["losses"]
    assert "edges" not in plain and not hasattr(plain["model"].linear_mapper, "edge_mask")


def test_graphed_run_holds_pruned_edges_at_zero(tmp_path):
    run = _train("cheby", ["--graph"], tmp_path)
    _check_pruned_state(run, "cheby")
    eager = _train("cheby", [], tmp_path)
    print("losses:", eager["losses"], run["losses"])
    assert run["losses"][:PRUNE_STEP - 1] == pytest.approx(eager["losses"][:PRUNE_STEP - 1], rel=1e-4)


def test_refusals():
    import train
    with pytest.raises(SystemExit, match="--prune is not combined with --dp: every rank would score its own shard"):
        train.main(train.parse(["--model-type", "cheby", "--synthetic", "--prune", "3:0.5", "--dp"]))
    with pytest.raises(SystemExit, match="--prune: model type\\(s\\) sine have no edge-activation statistic to prune by"):
        train.main(train.parse(["--model-type", "sine", "--synthetic", "--prune", "3:0.5"]))

"""CPU-only checks of the C-ABI refusals of the three batch entry points (csrc/batch_u8.hip: kanvit_augment_u8, kanvit_mix_u8,
kanvit_resample_u8): every check their shared host path makes (batch_check_shape, batch_check_operands) and the table rule each adds,
by return code and full message text.  Nothing is launched: a refused call dereferences no pointer, and neither does an empty batch."""
import pytest

P = 0x1000          # a non-null dummy pointer, aligned to 16 bytes
POINTERS = {"images", "labels", "idx", "lut", "crop", "partner", "weight", "box", "out", "y_out", "y2_out", "w_out", "params_out"}
SHAPE = dict(N=3, B=2, H=4, W=4, C=1)
# a valid call per entry point, in the order of its C arguments (the stream, last, is null)
VALID = {
    "kanvit_augment_u8": dict(images=P, labels=P, idx=P, lut=P, out=P, y_out=P, params_out=P, **SHAPE, pad_y=1, pad_x=1, flip=1, seed=0, epoch=0),
    "kanvit_mix_u8": dict(images=P, labels=P, idx=P, lut=P, partner=P, weight=P, box=P, out=P, y_out=P, y2_out=P, w_out=P, **SHAPE, pad_y=1,
                          pad_x=1, flip=1, seed=0, epoch=0),
    "kanvit_resample_u8": dict(images=P, labels=P, idx=P, lut=P, crop=P, partner=P, weight=P, box=P, out=P, y_out=P, y2_out=P, w_out=P, **SHAPE,
                               OH=8, OW=8),
}


@pytest.fixture(scope="module")
def lib():
    from kanvit import build
    build.build(verbose=False)
    from kanvit import _lib
    return _lib.lib()


def _call(lib, fn, **kw):
    args = dict(VALID[fn], **kw)
    assert set(kw) <= set(VALID[fn])
    return getattr(lib, fn)(*[(v or None) if k in POINTERS else v for k, v in args.items()], None)


A, M, R = "kanvit_augment_u8", "kanvit_mix_u8", "kanvit_resample_u8"
REFUSALS = [
    # the dataset's shape (batch_check_shape) and what each entry point adds to it
    (A, dict(N=0), "kanvit_augment_u8: N=0: the dataset holds at least one image"),
    (M, dict(N=0), "kanvit_mix_u8: N=0: the dataset holds at least one image"),
    (R, dict(N=0), "kanvit_resample_u8: N=0: the dataset holds at least one image"),
    (A, dict(C=5), "kanvit_augment_u8: C=5 must be in 1..4 (the look-up table is staged as C x 1 KB)"),
    (M, dict(C=5), "kanvit_mix_u8: C=5 must be in 1..4 (the look-up table is staged as C x 1 KB)"),
    (R, dict(C=5), "kanvit_resample_u8: C=5 must be in 1..4 (the look-up table is staged as C x 1 KB)"),
    (A, dict(H=0), "kanvit_augment_u8: H=0, W=4 must be in 1..2^20"),
    (M, dict(H=0), "kanvit_mix_u8: H=0, W=4 must be in 1..2^20"),
    (R, dict(H=0), "kanvit_resample_u8: H=0, W=4 must be in 1..2^20"),
    (A, dict(pad_y=5), "kanvit_augment_u8: pad_y=5 must be in 0..H=4"),
    (M, dict(pad_y=5), "kanvit_mix_u8: pad_y=5 must be in 0..H=4"),
    (R, dict(OH=0), "kanvit_resample_u8: OH=0, OW=8 must be in 1..2^20"),
    # the batch size and the pointers (batch_check_operands)
    (A, dict(B=-1), "kanvit_augment_u8: B=-1 is negative"),
    (M, dict(B=-1), "kanvit_mix_u8: B=-1 is negative"),
    (R, dict(B=-1), "kanvit_resample_u8: B=-1 is negative"),
    (A, dict(flip=2), "kanvit_augment_u8: flip=2 is 0 (never) or 1 (with probability 1/2)"),
    (M, dict(flip=2), "kanvit_mix_u8: flip=2 is 0 (never) or 1 (with probability 1/2)"),
    (A, dict(out=0), "kanvit_augment_u8: null images/idx/lut/out"),
    (M, dict(out=0), "kanvit_mix_u8: null images/idx/lut/out"),
    (R, dict(out=0), "kanvit_resample_u8: null images/idx/lut/out"),
    (A, dict(labels=0), "kanvit_augment_u8: y_out without labels"),
    (M, dict(labels=0), "kanvit_mix_u8: y_out / y2_out without labels"),
    (R, dict(labels=0), "kanvit_resample_u8: y_out / y2_out without labels"),
    (A, dict(out=P + 2), "kanvit_augment_u8: a pointer is not aligned to its element size"),
    (M, dict(out=P + 2), "kanvit_mix_u8: a pointer is not aligned to its element size"),
    (R, dict(out=P + 2), "kanvit_resample_u8: a pointer is not aligned to its element size"),
    # the mix tables: all three for kanvit_mix_u8, all three or none for kanvit_resample_u8
    (M, dict(weight=0), "kanvit_mix_u8: null partner/weight/box (the three tables come together)"),
    (R, dict(weight=0), "kanvit_resample_u8: null weight (the three mix tables partner/weight/box come together or not at all)"),
]


@pytest.mark.parametrize("fn,kw,message", REFUSALS, ids=[f"{fn[7:]}-{k}={v}" for fn, kw, _ in REFUSALS for k, v in kw.items()])
def test_refusal_code_and_message(lib, fn, kw, message):
    assert _call(lib, fn, **kw) == -22
    assert lib.kanvit_last_error().decode() == message


@pytest.mark.parametrize("fn", [A, M, R])
def test_empty_batch_returns_0_with_every_pointer_null(lib, fn):
    assert _call(lib, fn, B=0, **{k: 0 for k in VALID[fn] if k in POINTERS}) == 0

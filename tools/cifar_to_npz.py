"""Convert an already unpacked CIFAR-10 / CIFAR-100 "python version" directory into the .npz layout of kanvit/data.py
(train.py --data-npz): x_train / x_test uint8 [N, 32, 32, 3], y_train / y_test int64, mean / std float32 [3].

    python tools/cifar_to_npz.py cifar-100-python cifar100.npz
    python tools/cifar_to_npz.py cifar-10-batches-py cifar10.npz

The directory is what the dataset's own archive unpacks to: `train` and `test` (CIFAR-100, fine labels) or `data_batch_1..5` and
`test_batch` (CIFAR-10).  This tool reads local files only; it has no download option.  CIFAR-100 gets the mean and std the reference
normalises with (train.py:101-104); CIFAR-10's are computed from its training images."""
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kan-vit_amd"))

CIFAR100_MEAN, CIFAR100_STD = [0.5071, 0.4867, 0.4408], [0.2675, 0.2565, 0.2761]


def _read(path):
    with open(path, "rb") as f:
        d = pickle.load(f, encoding="bytes")
    labels = d[b"fine_labels"] if b"fine_labels" in d else d[b"labels"]
    x = np.asarray(d[b"data"], dtype=np.uint8).reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1)      # rows are channel-planar
    return np.ascontiguousarray(x), np.asarray(labels, dtype=np.int64)


def convert(src):
    if os.path.exists(os.path.join(src, "train")):
        (xt, yt), (xe, ye) = _read(os.path.join(src, "train")), _read(os.path.join(src, "test"))
        mean, std = np.array(CIFAR100_MEAN, np.float32), np.array(CIFAR100_STD, np.float32)
    elif os.path.exists(os.path.join(src, "data_batch_1")):
        parts = [_read(os.path.join(src, f"data_batch_{i}")) for i in range(1, 6)]
        xt, yt = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        xe, ye = _read(os.path.join(src, "test_batch"))
        from kanvit.data import channel_stats
        mean, std = channel_stats(xt)
    else:
        raise SystemExit(f"{src}: neither 'train' (CIFAR-100) nor 'data_batch_1' (CIFAR-10) found; unpack the python version of the dataset there")
    return dict(x_train=xt, y_train=yt, x_test=xe, y_test=ye, mean=mean, std=std)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 2:
        raise SystemExit(__doc__)
    arrays = convert(argv[0])
    np.savez(argv[1], **arrays)
    print(f"{argv[1]}: {len(arrays['x_train'])} training and {len(arrays['x_test'])} test images")


if __name__ == "__main__":
    main()

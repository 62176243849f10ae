"""Worker for tests/test_gpu_conv_oracle.py::test_wgrad_1x1_plain: wgrad1x1_kernel (W1_PLAIN) is
planned only when SDX_W1_PIPE=0 is read at process start (or for tensors of 2^31 elements), so
its rows run in a fresh process with that environment: the rows of test_wgrad_1x1 on the two
smallest shapes that take both loader layouts (bn 128: two chunks per thread, bn 256: three)."""
import os
import signal
import sys

TESTS = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(TESTS), TESTS]

import torch  # noqa: E402

import conv_checks as K  # noqa: E402

SHAPES = [(K._w1(1, 8, 128, 128, 1), 128), (K._w1(1, 8, 256, 128, 1), 256)]
MARKER = "W1-PLAIN-OK"


def main():
    signal.alarm(150)       # the worker's own limit: SIGALRM ends it
    assert os.environ.get("SDX_W1_PIPE") == "0", "knob not set"
    from simclr_pytorch_distributed_amd.ops import _ext
    impl = K.ExtImpl(_ext.require(), torch.device("cuda:0"))
    for shape, bn in SHAPES:
        p = K.plan(impl.m, "wgrad", shape, 10)
        assert p["variant"] == "plain", (shape, p["variant"])
        assert p["bn"] == bn, (shape, p["bn"])
        K.wgrad_row(impl, shape, 10, p["steps"])
    torch.cuda.synchronize()
    print(MARKER)


if __name__ == "__main__":
    main()

"""Record tests/golden/generator_operands/*.npz: what the beta-CEM generator
kernels wrote, per step of tests/generator_operands.py's walk, on an MI355X
with the library built from commit

    14b9b93  Declare each handle buffer once (buffers.hpp); split mpcmmd.hip by role

-- the last build whose k_belite stored the U rows of the generators as a
second fp64 plane of ``gen`` and whose samplers walked the padding block.
tests/test_gpu_generator_operands.py holds every later build to these bits.

One file per (case, step), each well under the 1 MiB limit for committed
files.  Run on the GPU machine, from a checkout of that commit (or with
MPCMMD_LIB naming its libmpcmmd.so):

    python tests/golden/make_generator_operands_golden.py [output directory]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mpc-mmd_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

PARENT = "14b9b93"


def main():
    from optimizer import _native
    import generator_operands as go
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "generator_operands")
    os.makedirs(dst, exist_ok=True)
    for n, B, genwave in go.CASES:
        if genwave is None:
            os.environ.pop("MPCMMD_GENWAVE", None)
        else:
            os.environ["MPCMMD_GENWAVE"] = genwave
        steps, info = go.walk(_native, n, B)
        for step, arrays in steps.items():
            path = os.path.join(dst, f"{go.case_id(n, B)}_{step}.npz")
            np.savez_compressed(path, parent=np.array(PARENT), gen_wave=np.array(info["gen_wave"]), **arrays)
            print(path, os.path.getsize(path), "bytes", info, flush=True)


if __name__ == "__main__":
    main()

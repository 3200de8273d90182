"""Writes tests/golden/jpeg_host_answers_v1.npz: what the host decoder (mrcnn_jpeg_coefficients with entropy = HOST) answers on the 25
files of tests/jpeg_entropy_cases.py, each intact and in its 25 damaged(data, seed=len(data)) variants — 650 answers.  Every other
JPEG test takes the host decoder as its expectation; this pins the decoder itself, on damaged input above all.

    MRCNN_HIP_LIB=<the library of the commit whose answers are to be kept> python tests/golden/make_jpeg_host_answers.py

Run it against the library of the commit BEFORE a change to the decoder, in a scratch worktree (git worktree add, make -C
mask-rcnn-coreml_amd/csrc), never against the tree under test.  Arrays, rows in sorted(files()) order, column 0 the intact file and
columns 1..25 the damaged variants in damaged()'s order:
    names     [25]       the file names
    status    [25, 26]   int8: the MRCNN_* status
    message   [25, 26]   int16: index into `messages` ("" where the status is OK)
    crc       [25, 26]   uint32: zlib.crc32 of the int16 coefficient array where the status is OK, else 0
    messages  [M]        the distinct messages, sorted"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def answers(K):
    """[(name, [(label, status, message, crc)] * 26)] from the library that is loaded."""
    out = []
    for name in sorted(K.files()):
        data = K.files()[name]
        row = []
        for label, variant in [("intact", data)] + K.damaged(data, seed=len(data)):
            st, msg, coef, _ = K.coefficients([variant], K.HOST)
            row.append((label, int(st), msg, zlib.crc32(coef.tobytes()) if st == 0 else 0))
        out.append((name, row))
    return out


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import jpeg_entropy_cases as K
    rows = answers(K)
    messages = sorted({m for _, row in rows for _, _, m, _ in row})
    index = {m: i for i, m in enumerate(messages)}
    path = os.path.join(HERE, "jpeg_host_answers_v1.npz")
    np.savez_compressed(path, names=np.array([n for n, _ in rows]), status=np.array([[r[1] for r in row] for _, row in rows], np.int8),
                        message=np.array([[index[r[2]] for r in row] for _, row in rows], np.int16),
                        crc=np.array([[r[3] for r in row] for _, row in rows], np.uint32), messages=np.array(messages))
    print(f"{path}: {sum(len(row) for _, row in rows)} answers, {len(messages)} distinct messages, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()

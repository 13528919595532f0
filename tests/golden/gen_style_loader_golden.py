#!/usr/bin/env python3
"""Generate tests/golden/g15_style_loader.npz by running the REFERENCE's frame-ordered loader.

Run where the reference tree is present (see ref_shim.py):
    python tests/golden/gen_style_loader_golden.py

The reference's `LightDataLoader(shuffle=False).loss_coh_get_batch` (dataset.py:734-779) walks a data set by (style,
frame, start).  Here it is run over a stub data set that answers `getitem_forlosscoh(idx, style, frame)` with the three
integers it was asked for, and the (style, frame, pixels) of every call are recorded as data.  No reference source is
copied; the fixture holds integers.  tests/test_style_train_cpu.py replays train_data.CoherenceCursor against it."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_shim  # noqa: E402

_saved = ref_shim.install()
import dataset as ref_dataset  # noqa: E402

ref_shim.restore_env(_saved)

# (S, F, h, w, B, calls): none of them reaches the loader's reset at start + B >= S*F*h*w
CASES = [(2, 3, 4, 5, 8, 40), (1, 3, 4, 5, 8, 20), (3, 2, 3, 3, 4, 40)]


class Stub:
    """What LightDataLoader reads of a data set: len, frame_num, style_num, h, w, item 0's keys, getitem_forlosscoh."""

    def __init__(self, S, F, h, w):
        self.style_num, self.frame_num, self.h, self.w = S, F, h, w

    def __len__(self):
        return self.style_num * self.frame_num * self.h * self.w

    def __getitem__(self, idx):
        return self.getitem_forlosscoh(idx, 0, 0)

    def getitem_forlosscoh(self, idx, style_id, frame_id):
        return {"style_id": np.int64(style_id), "frame_id": np.int64(frame_id), "pixel": np.int64(idx % (self.h * self.w))}


def main():
    out = {"cases": np.array(CASES, np.int64)}
    for k, (S, F, h, w, B, calls) in enumerate(CASES):
        loader = ref_dataset.LightDataLoader(Stub(S, F, h, w), batch_size=B, shuffle=False)
        rows = []
        for _ in range(calls):
            b = loader.loss_coh_get_batch()
            sid, fid, pix = (b[key].numpy().astype(np.int64) for key in ("style_id", "frame_id", "pixel"))
            assert (sid == sid[0]).all() and (fid == fid[0]).all()
            rows.append(np.concatenate([[sid[0], fid[0]], pix]))
        out["case%d" % k] = np.stack(rows)          # [calls, 2 + B]: style, frame, the B pixels
    path = os.path.join(HERE, "g15_style_loader.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate tests/golden/fiducial.json from the reference's test DATA under testdata/board/ (style of make_fixtures.py).

Needs the reference checkout's testdata (REF in make_fixtures.py). The output is data only:
  * images   marker-expected.png (id 471, 500 px), locked-marker-expected.png (750 px) and board.png (690 x 1050) hold the two
             grey levels 0 and 255 only: stored as run lengths over the flattened image ({"shape", "first", "runs"}).
  * watermark  of wartermark-marker-expected.png the pixels that are neither 0 nor 255 as [y, x, value] ("grey"), and where it is 255
             as run lengths ("white"); every other pixel is 0.
  * boards   ids and corners of defaultBoard- / chessBoard- / frameBoard-expected.yml, board_pix.yml and board_meters.yml.
No reference source text is copied; only test inputs and expected outputs.
"""
import json
import os
import sys

import numpy as np
from PIL import Image

from make_fixtures import REF, OUT, board_conf


def run_lengths(img):
    flat = img.reshape(-1)
    assert set(np.unique(flat).tolist()) <= {0, 255}
    edges = np.flatnonzero(np.diff(flat)) + 1
    bounds = np.concatenate(([0], edges, [flat.size]))
    return {"shape": list(img.shape), "first": int(flat[0]), "runs": [int(v) for v in np.diff(bounds)]}


def gray(name):
    img = np.asarray(Image.open(os.path.join(REF, "board", name)))
    assert img.dtype == np.uint8 and img.ndim == 2, (name, img.dtype, img.shape)
    return img


def main():
    if not os.path.isdir(REF):
        sys.exit("reference testdata not available; fixtures are already committed")
    wm = gray("wartermark-marker-expected.png")
    ys, xs = np.nonzero((wm != 0) & (wm != 255))
    doc = {
        "source": "testdata/board/",
        "marker": {"id": 471, "size": 500},
        "images": {"marker": run_lengths(gray("marker-expected.png")), "locked_marker": run_lengths(gray("locked-marker-expected.png")),
                   "board": run_lengths(gray("board.png"))},
        "watermark": {"white": run_lengths(np.where(wm == 255, 255, 0).astype(np.uint8)), "grey":[[int(y), int(x), int(wm[y, x])] for y, x in zip(ys, xs)]},
        "boards": {name: board_conf(os.path.join(REF, "board", f)) for name, f in (
            ("default", "defaultBoard-expected.yml"), ("chessboard", "chessBoard-expected.yml"), ("frame", "frameBoard-expected.yml"),
            ("board_pix", "board_pix.yml"), ("board_meters", "board_meters.yml"))},
    }
    with open(os.path.join(OUT, "fiducial.json"), "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()

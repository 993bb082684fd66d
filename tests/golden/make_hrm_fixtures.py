#!/usr/bin/env python3
"""Generate the HRM board fixtures under tests/golden/ from the reference's test DATA (style of make_fixtures.py).

Needs the reference checkout's testdata (REF in make_fixtures.py). Outputs are data:
  * board4x4.pgm   testdata/hrm/boards/board4x4.png, the 8-bit gray board image HighlyReliableMarkers::createBoardImage made from
                   the first 16 markers of d4x4_100 (hrm.json's dictionary) on a 4 x 4 grid.
  * board4x4.json  testdata/hrm/boards/board4x4.yml: the board configuration written with it (ids, corners in pixels). Its ids come
                   from an older getId() (1 << pos), half of what the current one (2 << pos) gives.
No reference source text is copied; only test inputs and expected outputs.
"""
import json
import os

import numpy as np
from PIL import Image

from make_fixtures import REF, OUT, board_conf, write_pgm


def main():
    img = np.asarray(Image.open(os.path.join(REF, "hrm/boards/board4x4.png")))
    assert img.dtype == np.uint8 and img.ndim == 2
    write_pgm(os.path.join(OUT, "board4x4.pgm"), img)
    doc = {"source_png": "hrm/boards/board4x4.png", "source_yml": "hrm/boards/board4x4.yml", "grid": [4, 4], "n": 4,
           "dictionary": "hrm.json: dictionary.markers[0:16]", "board": board_conf(os.path.join(REF, "hrm/boards/board4x4.yml"))}
    with open(os.path.join(OUT, "board4x4.json"), "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()

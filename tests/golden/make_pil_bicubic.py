"""Golden vectors for preprocess_image's resize (common/data_utils.py:450): `image.resize(model_input_shape[::-1], Image.BICUBIC)` on
8-bit RGB.  This script makes the same PIL call on the seeded inputs of tests/pil_rules.py (CASES x KINDS, regenerated from the seed by
the tests: only Pillow's outputs are stored); run where Pillow is installed (12.2.0 when this file was made):
python tests/golden/make_pil_bicubic.py  ->  tests/golden/pil_bicubic.npz"""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pil_rules  # noqa: E402

out = {}
for i, (hw, HW) in enumerate(pil_rules.CASES):
    for kind in pil_rules.KINDS:
        im = Image.fromarray(pil_rules.case_input(hw, kind))
        out['out%d_%s' % (i, kind)] = np.asarray(im.resize(HW[::-1], Image.BICUBIC))
np.savez_compressed(os.path.join(HERE, 'pil_bicubic.npz'), **out)
print('wrote', len(out), 'arrays')

"""Import-path shim: `from deeplabv3p.data import SegmentationGenerator` works as in the reference (train.py:14); the class lives in
tf-keras-deeplabv3p-model-set_amd/data.py."""
import importlib as _il

_m = _il.import_module('tf-keras-deeplabv3p-model-set_amd.data')
SegmentationGenerator = _m.SegmentationGenerator

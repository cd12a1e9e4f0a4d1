"""Import-path shim: `from deeplab import DeepLab` works as with the reference's deeplab.py; everything lives in
tf-keras-deeplabv3p-model-set_amd/inference.py.  segment_video and the command line are not built (they need cv2)."""
import importlib as _il

_i = _il.import_module('tf-keras-deeplabv3p-model-set_amd.inference')
DeepLab = _i.DeepLab

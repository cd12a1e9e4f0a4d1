"""Import-path shim: `from fast_scnn.model import get_fast_scnn_model` works as in the reference (train.py:150-164);
everything lives in tf-keras-deeplabv3p-model-set_amd/."""

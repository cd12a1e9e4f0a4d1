"""Import-path shim: `from unet.model import get_unet_model` works as in the reference (train.py:150-164);
everything lives in tf-keras-deeplabv3p-model-set_amd/."""

import importlib as _il

_m = _il.import_module('tf-keras-deeplabv3p-model-set_amd.model')
_u = _il.import_module('tf-keras-deeplabv3p-model-set_amd.unet')
get_unet_model = _m.get_unet_model
unet_model_map = _u.unet_model_map

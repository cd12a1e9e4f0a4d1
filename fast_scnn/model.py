import importlib as _il

_m = _il.import_module('tf-keras-deeplabv3p-model-set_amd.model')
_f = _il.import_module('tf-keras-deeplabv3p-model-set_amd.fast_scnn')
get_fast_scnn_model = _m.get_fast_scnn_model
fast_scnn_model_map = _f.fast_scnn_model_map

"""The reference's third driver, deeplab.py, on the device: `DeepLab(**kwargs).segment_image(image)`, `.predict(image_data, image_shape)`
and `.dump_model_file(path)`, with the helpers it takes from common/ (create_pascal_label_colormap, label_to_color_image,
preprocess_image, mask_resize) under their names and contracts.

A frame goes up once as bytes and stays on the device: Pillow's bicubic resize to the model's input (augment.pil_resize, pinned
against Pillow), normalisation (Executor.set_inputs), the forward pass with the argmax taken on the device (Executor.eval_step), and
one launch that takes the mask back to the frame's size by cv2's INTER_NEAREST rule, colours it and blends it over the frame
(dl3p_mask_overlay_u8).  Nothing synchronises in between; `segment_batch` is that chain for N frames, `predict` and `segment_image`
are the reference's signatures on top of it.

The overlay is NOT the reference's picture: visualize_segmentation (common/utils.py:266-340) draws through matplotlib onto a
1000 x 1000 canvas with a legend.  What is kept is its per-pixel composite `imshow(image); imshow(mask_image, alpha=overlay)` at the
frame's own resolution, as the integer rule (img (256 - A) + colour A + 128) >> 8 with A = rint(overlay * 256).

Dense-CRF post-processing runs on the device between the class ids and the resize back to the frame (`dense_crf=True`, ops.dense_crf:
the reference's crf_postprocess with every filter computed exactly).  `do_crf=True` still raises: that switch names pydensecrf's
permutohedral-lattice approximation, which is not built.

Not built: the lattice approximation behind `do_crf`, `segment_video` and the argparse `main` (they need cv2's capture and window),
`dump_saved_model` (TensorFlow's SavedModel)."""
import functools
import os

import numpy as np

from . import augment, ops
from ._lib import lib
from .model import batch_input, get_deeplabv3p_model, get_fast_scnn_model, get_unet_model, single_pass

OVERLAY = 0.7               # visualize_segmentation's default alpha


def get_classes(classes_path):
    """one class name per line (common/utils.py get_classes)"""
    with open(classes_path) as f:
        return [line.strip() for line in f.readlines()]


def create_pascal_label_colormap():
    """the PASCAL VOC colour map, (256, 3) int: the bits of the label index dealt out to R, G, B in turn, most significant colour
    bit first (label 1 -> (128, 0, 0), 2 -> (0, 128, 0), 3 -> (128, 128, 0), ...)"""
    index = np.arange(256, dtype=int)
    colormap = np.zeros((256, 3), dtype=int)
    for bit in range(8):
        colormap |= ((index[:, None] >> (3 * bit + np.arange(3)[None, :])) & 1) << (7 - bit)
    return colormap


def label_to_color_image(label):
    """(H, W) integer labels -> (H, W, 3) colours of the PASCAL map; ValueError for another rank or a label past the map"""
    label = np.asarray(label)
    if label.ndim != 2:
        raise ValueError('label_to_color_image takes a rank-2 label array, got rank %d' % label.ndim)
    colormap = create_pascal_label_colormap()
    if np.max(label) >= len(colormap):
        raise ValueError('label %d is past the %d entries of the colour map' % (np.max(label), len(colormap)))
    return colormap[label]


def _device_u8(a):
    """a dense CUDA uint8 tensor of `a` (NumPy array, PIL image or tensor): one upload if it is on the host"""
    import torch
    if not isinstance(a, torch.Tensor):
        a = np.asarray(a)
        if not (a.flags.c_contiguous and a.flags.writeable):    # (np.asarray of a PIL image is read-only: torch wants its own copy)
            a = np.array(a, order='C')
        a = torch.from_numpy(a)
    if a.dtype != torch.uint8:
        raise ValueError('expected 8-bit pixels, got %s' % (a.dtype,))
    return a.cuda(non_blocking=True).contiguous()


def preprocess_image(image, model_input_shape):
    """common/data_utils.py:436-454: a PIL image or an (h, w, 3) uint8 array -> (1, H, W, 3) float32 in [-1, 1]:
    Image.resize(model_input_shape[::-1], Image.BICUBIC) (on the device, bit for bit Pillow's bytes), then normalize_image"""
    frame = _device_u8(image)
    if frame.dim() != 3 or frame.shape[2] != 3:
        raise ValueError('preprocess_image takes an 8-bit RGB image, got shape %r' % (tuple(frame.shape),))
    resized = augment.pil_resize(frame[None], tuple(model_input_shape)).cpu().numpy()
    return resized.astype(np.float32) / 127.5 - 1


def overlay_tables(H, W, h0, w0):
    """the w0 + h0 integers dl3p_mask_overlay_u8 takes, nx[w0] then ny[h0]: cv2.INTER_NEAREST's source column / row in a (H, W) mask
    of every column / row of an (h0, w0) frame"""
    return np.concatenate([augment.nearest_axis(w0, W), augment.nearest_axis(h0, H)]).astype(np.int32)


@functools.lru_cache(maxsize=8)
def _overlay_consts(device, H, W, h0, w0):
    """overlay_tables and the colour map as bytes on `device`, kept per size pair like augment.pil_resize's tables"""
    import torch
    return (torch.as_tensor(overlay_tables(H, W, h0, w0)).to(device),
            torch.as_tensor(create_pascal_label_colormap().astype(np.uint8)).to(device))


def _mask_overlay(pred, frames, n_valid, shape, overlay=OVERLAY):
    """pred (N, H, W) int32 CUDA class ids, frames (N, h0, w0, 3) dense CUDA uint8 or None (no overlay), shape = (h0, w0)
    -> (masks (N, h0, w0) uint8, overlays (N, h0, w0, 3) uint8 or None), one launch on the current stream"""
    import torch
    N, H, W = pred.shape
    h0, w0 = shape
    dev = pred.device
    tab, cmap = _overlay_consts(dev, H, W, h0, w0)
    masks = torch.empty((N, h0, w0), dtype=torch.uint8, device=dev)
    overlays = torch.empty((N, h0, w0, 3), dtype=torch.uint8, device=dev) if frames is not None else None
    lib().mask_overlay_u8(pred.data_ptr(), frames.data_ptr() if frames is not None else None, masks.data_ptr(),
                          overlays.data_ptr() if frames is not None else None, tab.data_ptr(), cmap.data_ptr(), int(n_valid),
                          int(np.rint(overlay * 256)), N, H, W, h0, w0, torch.cuda.current_stream().cuda_stream)
    return masks, overlays


def mask_resize(mask, target_size):
    """common/data_utils.py:457-477: cv2.resize(mask, target_size, interpolation=cv2.INTER_NEAREST) of an (H, W) class mask;
    target_size = (width, height).  -> uint8 (height, width)"""
    import torch
    mask = np.asarray(mask)
    if mask.ndim != 2:
        raise ValueError('mask_resize takes a rank-2 mask, got rank %d' % mask.ndim)
    pred = torch.from_numpy(np.ascontiguousarray(mask.astype(np.int32))).cuda()[None]
    return _mask_overlay(pred, None, 0, (int(target_size[1]), int(target_size[0])))[0][0].cpu().numpy()


class DeepLab(object):
    """deeplab.py:43-113 with the reference's keyword arguments.  `weights_path=None` builds a randomly initialised model (the
    reference cannot); `dense_crf=True` (or a dict of ops.dense_crf's keyword arguments) refines every mask with the exact dense CRF on
    the device; `do_crf=True` raises: pydensecrf's lattice approximation is not built."""
    _defaults = {
        'model_type': 'mobilenetv2_lite',
        'classes_path': os.path.join('configs', 'voc_classes.txt'),
        'model_input_shape': (512, 512),
        'output_stride': 16,
        'weights_path': os.path.join('weights', 'mobilenetv2_original.h5'),
        'do_crf': False,
        # DeepLab's multi-scale / mirrored protocol (not the reference's deeplab.py, which predicts one scale): the defaults keep the
        # single unmirrored pass
        'scales': (1.0,),
        'flip': False,
        # the fully connected CRF on the device (ops.dense_crf): False, True (the reference's parameters) or a dict of its keywords
        'dense_crf': False,
    }

    def __init__(self, **kwargs):
        for key, value in {**self._defaults, **kwargs}.items():       # (keys beyond the defaults are kept as attributes, as there)
            setattr(self, key, value)
        if self.do_crf:
            raise ValueError('do_crf=True names the CRF of deeplabv3p/postprocess_np.py as pydensecrf filters it, on a permutohedral '
                             'lattice; that approximation is not built.  dense_crf=True runs the same CRF with exact filters on the '
                             'device')
        self.model_input_shape = tuple(int(v) for v in self.model_input_shape)
        self.class_names = get_classes(self.classes_path)
        self.crf_params = ops.crf_params(self.dense_crf, len(self.class_names))     # (refused before the model is built)
        self.deeplab_model = self._generate_model()
        if not single_pass(self.scales, self.flip):
            self.scales = self.deeplab_model.tta_scales(self.scales)

    def _refine(self, pred, x):
        """the dense CRF over the class ids `pred` (N, H, W) with the images `x` at the model's size: CUDA bytes, or normalised
        float32 that go back to bytes by the reference's denormalize_image"""
        import torch
        if self.crf_params is None:
            return pred
        if not (isinstance(x, torch.Tensor) and x.dtype == torch.uint8):
            x = ops.denormalize_u8(torch.as_tensor(np.asarray(x, dtype=np.float32)).cuda(non_blocking=True))
        return ops.dense_crf(x, pred, len(self.class_names), **self.crf_params)

    def _generate_model(self):
        num_classes = len(self.class_names)
        if num_classes > 253:
            raise ValueError('%s names %d classes; a PNG label map holds at most 253' % (self.classes_path, num_classes))
        weights_path = self.weights_path
        if weights_path is not None:
            weights_path = os.path.expanduser(weights_path)
            if not weights_path.endswith('.h5'):
                raise ValueError('weights_path must name a Keras .h5 file (got %r)' % (weights_path,))
        # the factory train.py:161-166 picks by the model type's prefix
        if self.model_type.startswith('unet_'):
            return get_unet_model(self.model_type, num_classes, self.model_input_shape, weights_path=weights_path, training=False)
        if self.model_type.startswith('fast_scnn'):
            return get_fast_scnn_model(self.model_type, num_classes, self.model_input_shape, weights_path=weights_path, training=False)
        return get_deeplabv3p_model(self.model_type, num_classes, model_input_shape=self.model_input_shape,
                                    output_stride=self.output_stride, freeze_level=0, weights_path=weights_path, training=False)

    def _class_ids(self, x):
        """x: (N, H, W, 3) bytes (CUDA) or normalised float32 (host) at the model's size -> (N, H, W) int32 CUDA class ids"""
        H, W = self.model_input_shape
        if tuple(x.shape[1:]) != (H, W, 3):
            raise ValueError('the model takes (N, %d, %d, 3) images, got %r' % (H, W, tuple(x.shape)))
        return self.deeplab_model.class_ids(x, scales=self.scales, flip=self.flip)      # (multi-scale: the frames are bytes then)

    def segment_batch(self, frames):
        """frames (N, h0, w0, 3) uint8, NumPy or a CUDA tensor -> (masks (N, h0, w0), overlays (N, h0, w0, 3)), CUDA uint8 tensors:
        the class mask at the frames' size (mask_resize of the prediction) and the colour-mapped mask blended over the frames.  One
        upload if `frames` is on the host, then everything on the current stream with nothing synchronising in between."""
        frames = _device_u8(frames)
        if frames.dim() != 4 or frames.shape[3] != 3:
            raise ValueError('segment_batch takes (N, h, w, 3) 8-bit RGB frames, got shape %r' % (tuple(frames.shape),))
        x = augment.pil_resize(frames, self.model_input_shape)
        pred = self._refine(self._class_ids(x), x)
        return _mask_overlay(pred, frames, len(self.class_names), tuple(frames.shape[1:3]))

    def predict(self, image_data, image_shape):
        """deeplab.py:96-109: image_data (1, H, W, 3), normalised float32 (what preprocess_image returns) or uint8; image_shape =
        (height, width) of the original image -> the class mask at that size, uint8 (height, width) NumPy"""
        if isinstance(image_data, (list, tuple)):
            image_data = image_data[0]
        x = batch_input(image_data)
        if isinstance(x, np.ndarray) and x.dtype == np.uint8:       # (bytes on the host go up as bytes)
            x = _device_u8(x)
        pred = self._refine(self._class_ids(x), x)
        masks, _ = _mask_overlay(pred, None, len(self.class_names), (int(image_shape[0]), int(image_shape[1])))
        return masks[0].cpu().numpy()

    def segment_image(self, image):
        """deeplab.py:81-93: a PIL image -> a PIL image of the same size, the segmentation blended over it"""
        from PIL import Image
        _, overlays = self.segment_batch(np.array(image.convert('RGB'))[None])
        return Image.fromarray(overlays[0].cpu().numpy())

    def dump_model_file(self, output_model_file):
        self.deeplab_model.save(output_model_file)

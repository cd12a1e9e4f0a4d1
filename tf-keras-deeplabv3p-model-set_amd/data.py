"""SegmentationGenerator (reference deeplabv3p/data.py:14-160) with the byte work on the device.

Per image, as the reference: PIL decode on the host, then -- after ONE upload of the image and label bytes -- the twelve augmentations in
the reference's order (data.py:72-106), each through the augment.py function of the same name with N = 1 (so every decision,
random_crop's included, is drawn per image and in the reference's order from np.random / random), and the final resize straight into
slot n of a uint8 batch.  Everything is enqueued on the current stream; two batch buffers alternate, so the batch handed out last stays
untouched while the next one is built; nothing here synchronises.

random_zoom_rotate, random_histeq and the resize are UNPINNED restatements of OpenCV's 8-bit arithmetic (augment.py).

output='device' (default) yields uint8 CUDA tensors, images (B, H, W, 3) and labels (B, H*W, 1): Executor.set_inputs normalises the
pixels and remaps labels above num_classes - 1 to ignore_index on the device; with weighted_type='adaptive' the third item is the
string 'adaptive' (the balanced weights are then computed on the device as well).  output='numpy' downloads the batch and returns the
reference's contract: float32 images x / 127.5 - 1, float32 labels with the remap applied, and {'pred_mask': weights}."""
import os
import random
import time

import numpy as np


def balanced_weights(labels):
    """sklearn.utils.class_weight.compute_class_weight('balanced') per pixel (data.py:134-145): n / (k count_c) over the k values
    present in the image, float64 rounded to float32; labels (B, P) integers"""
    out = np.zeros(labels.shape, np.float32)
    for n, lab in enumerate(labels):
        classes, inverse, counts = np.unique(lab, return_inverse=True, return_counts=True)
        out[n] = (lab.size / (len(classes) * counts.astype(np.float64)))[inverse.reshape(-1)]
    return out


class SegmentationGenerator:
    def __init__(self, dataset_path, data_list,
                 batch_size=1,
                 num_classes=21,
                 input_shape=(512, 512),
                 weighted_type=None,
                 is_eval=False,
                 ignore_index=255,
                 augment=True,
                 output='device'):
        if output not in ('device', 'numpy'):
            raise ValueError("output must be 'device' or 'numpy'")
        dataset_realpath = os.path.realpath(dataset_path)
        self.image_path_list = [os.path.join(dataset_realpath, 'images', image_id.strip() + '.jpg') for image_id in data_list]
        self.label_path_list = [os.path.join(dataset_realpath, 'labels', image_id.strip() + '.png') for image_id in data_list]
        # initialize random seed (as the reference does)
        np.random.seed(int(time.time()))

        self.num_classes = num_classes
        self.batch_size = batch_size
        self.input_shape = tuple(input_shape)
        self.weighted_type = weighted_type
        self.augment = augment
        self.is_eval = is_eval
        self.ignore_index = ignore_index
        self.output = output
        self.device = 'cuda'                # (an attribute, not an argument: the host tests point it at 'cpu' under a stub library)
        self._bufs = [None, None]           # two alternating (images, labels) batches on the device
        self._k = 0

    def get_batch_image_path(self, i):
        return self.image_path_list[i * self.batch_size:(i + 1) * self.batch_size]

    def get_batch_label_path(self, i):
        return self.label_path_list[i * self.batch_size:(i + 1) * self.batch_size]

    def get_weighted_type(self):
        return self.weighted_type

    def __len__(self):
        return len(self.image_path_list) // self.batch_size

    @staticmethod
    def decode(image_path, label_path):
        """(h, w, 3) and (h, w) uint8 arrays, as the reference opens them (data.py:63-68)"""
        from PIL import Image
        img = Image.open(image_path).convert('RGB')
        lbl = Image.open(label_path)
        image = np.array(img)
        label = np.array(lbl)
        img.close()
        lbl.close()
        if label.dtype != np.uint8 or label.shape != image.shape[:2]:
            raise ValueError('%s: the label must be one uint8 plane of the image\'s size, got %s %s' % (label_path, label.dtype, label.shape))
        return image, label

    def upload(self, image, label):
        """one host -> device copy of the image bytes followed by the label bytes -> (1, h, w, 3), (1, h, w) uint8 tensors"""
        import torch
        h, w = label.shape
        dev = torch.from_numpy(np.concatenate([image.reshape(-1), label.reshape(-1)])).to(self.device)
        return dev[:h * w * 3].view(1, h, w, 3), dev[h * w * 3:].view(1, h, w)

    def augment_chain(self, image, label):
        """the reference's twelve steps (data.py:72-106), N = 1"""
        from . import augment as A
        image, label = A.random_horizontal_flip(image, label)
        image, label = A.random_vertical_flip(image, label)
        image, label = A.random_zoom_rotate(image, label)
        image, label = A.random_gridmask(image, label)
        image = A.random_brightness(image)
        image = A.random_chroma(image)
        image = A.random_contrast(image)
        image = A.random_sharpness(image)
        image = A.random_grayscale(image)
        image = A.random_blur(image)
        image, label = A.random_crop(image, label, self.input_shape, resize_small=True)
        image = A.random_histeq(image)
        return image, label

    def _batch(self):
        import torch
        slot = self._k & 1
        self._k += 1
        if self._bufs[slot] is None:
            H, W = self.input_shape
            self._bufs[slot] = (torch.empty((self.batch_size, H, W, 3), dtype=torch.uint8, device=self.device),
                                torch.empty((self.batch_size, H * W, 1), dtype=torch.uint8, device=self.device))
        return self._bufs[slot]

    def __getitem__(self, i):
        from . import augment as A
        batch_images, batch_labels = self._batch()
        for n, (image_path, label_path) in enumerate(zip(self.get_batch_image_path(i), self.get_batch_label_path(i))):
            image, label = self.upload(*self.decode(image_path, label_path))
            if self.augment:
                image, label = self.augment_chain(image, label)
            # Resize image & label mask to model input shape, into slot n of the batch
            A.resize(image, label, self.input_shape, out=(batch_images[n], batch_labels[n]))
        if self.output == 'device':
            if self.weighted_type == 'adaptive':
                return batch_images, batch_labels, 'adaptive'
            return batch_images, batch_labels
        return self.reference_contract(batch_images.cpu().numpy(), batch_labels.cpu().numpy())

    def reference_contract(self, images_u8, labels_u8):
        """what the reference's __getitem__ returns for a uint8 batch (data.py:113-154)"""
        images = images_u8.astype(np.float32) / 127.5 - 1
        labels = labels_u8.astype('int32')
        labels[labels > (self.num_classes - 1)] = self.ignore_index
        batch_labels = labels.astype('float32')
        if self.weighted_type == 'adaptive':
            return images, batch_labels, {'pred_mask': balanced_weights(labels.reshape(labels.shape[0], -1))}
        return images, batch_labels

    def on_epoch_end(self):
        # Shuffle dataset for next epoch
        c = list(zip(self.image_path_list, self.label_path_list))
        random.shuffle(c)
        self.image_path_list, self.label_path_list = zip(*c)

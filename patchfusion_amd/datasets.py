"""The reference's ``ImageDataset`` (estimator/datasets/general_dataset.py:145-230) over the device path: images through
``ImagePreprocessor`` (decoded and resized on the device), ground truth through ``groundtruth.read_depth_gt``.  Same constructor
arguments, the same sorted-listing pairing of image and ground-truth files, the same keys from ``__getitem__`` -- with every tensor on
the device -- and the same ``get_metrics`` arguments.  The training-side augmentations are not part of it."""
import os

import numpy as np
import torch

from . import postprocess
from .groundtruth import read_depth_gt
from .preprocess import ImagePreprocessor

U4K_IMAGE_SHAPE = (2160, 3840, 3)                               # general_dataset.py:24: the raw files of 'u4k' are B, G, R bytes


def _network_shape(network_process_size, multiple):
    """what midas.Resize(net_w, net_h, keep_aspect_ratio=False, ensure_multiple_of=m, resize_method='minimal') resizes to"""
    return tuple(int(np.round(int(v) / multiple) * multiple) for v in network_process_size[:2])


class ImageDataset:
    def __init__(self, rgb_image_dir, mode='', min_depth=1e-3, max_depth=80, gt_dir=None, image_resolution=[2160, 3840], dataset_name='',
                 network_process_size=(384, 512), resize_mode='zoe', device="cuda", ops=None):
        self.min_depth = min_depth
        self.max_depth = max_depth
        self.mode = mode
        self.rgb_image_dir = rgb_image_dir
        self.files = sorted(os.listdir(self.rgb_image_dir))
        self.gt_dir = gt_dir
        self.dataset_name = dataset_name
        if gt_dir is not None:
            self.gt_files = sorted(os.listdir(self.gt_dir))     # image and ground truth pair up by their position in the sorted listings
        if resize_mode == 'zoe':
            multiple = 32
        elif resize_mode == 'depth-anything':
            multiple = 14
        else:
            raise NotImplementedError
        self.image_resolution = image_resolution
        self.device = torch.device(device)
        self.ops = ops
        self.preprocess = ImagePreprocessor(image_resolution=tuple(image_resolution), process_shape=_network_shape(network_process_size, multiple),
                                            dataset_name=dataset_name, device=self.device, ops=ops)

    def __len__(self):
        return len(self.files)

    def _image(self, path):
        if self.dataset_name == 'u4k':                          # raw bytes, which ImagePreprocessor.read refuses: nothing to decode
            raw = np.fromfile(path, dtype=np.uint8)
            if raw.size != int(np.prod(U4K_IMAGE_SHAPE)):
                raise ValueError(f"{path}: a 'u4k' image holds {int(np.prod(U4K_IMAGE_SHAPE))} bytes, got {raw.size}")
            return self.preprocess(raw.reshape(U4K_IMAGE_SHAPE))
        return self.preprocess.read(path)

    def __getitem__(self, index):
        name = self.files[index]
        image = self._image(os.path.join(self.rgb_image_dir, name))
        filename = name.replace(".jpg", "").replace(".png", "").replace(".jpeg", "")
        ret = {'image_lr': image["image_lr"], 'image_hr': image["image_hr"]}
        if self.gt_dir is not None:
            gt = read_depth_gt(os.path.join(self.gt_dir, self.gt_files[index]), self.dataset_name, device=self.device, ops=self.ops)
            ret['depth_gt'] = gt.depth
            ret['boundary'] = gt.edge.unsqueeze(0)              # to_tensor of a 2-D array: [1,H,W]
        ret['img_file_basename'] = filename
        return ret

    def get_metrics(self, depth_gt, result, disp_gt_edges, **kwargs):
        return postprocess.compute_metrics(depth_gt, result, disp_gt_edges=disp_gt_edges, min_depth_eval=self.min_depth,
                                           max_depth_eval=self.max_depth, garg_crop=False, eigen_crop=False, dataset=self.dataset_name,
                                           ops=self.ops)

    def evaluator(self, capacity=64):
        """a DepthEvaluator with get_metrics' arguments: the same numbers without a host synchronisation per image"""
        return postprocess.DepthEvaluator(self.min_depth, self.max_depth, garg_crop=False, eigen_crop=False, dataset=self.dataset_name,
                                          capacity=capacity, ops=self.ops)

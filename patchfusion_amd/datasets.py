"""The reference's ``ImageDataset`` (estimator/datasets/general_dataset.py:145-230) over the device path: images through
``ImagePreprocessor`` (decoded and resized on the device), ground truth through ``groundtruth.read_depth_gt``.  Same constructor
arguments, the same sorted-listing pairing of image and ground-truth files, the same keys from ``__getitem__`` -- with every tensor on
the device -- and the same ``get_metrics`` arguments.

``UnrealStereo4kDataset`` (estimator/datasets/u4k_dataset.py) is the train and validation dataset of the reference's configs.  Any mode
but 'train' is the path above on the split file's pairs.  mode='train' adds the augmentations of transformers/augmentations.py on the
device (csrc/augment.hip): the host makes every random draw first, in the reference's order and from the same two generators, so a seeded
run yields the reference's sample and leaves Python's ``random`` and ``np.random`` in the reference's state; the image and the depth plane
are then rotated, flipped and colour-augmented in two launches, resized and cropped by the existing kernels.  Tensors live on the
device, so the class is used with ``num_workers=0``; ``collate_train`` stacks samples into the arguments of ``PatchFusion(mode='train')``."""
import math
import os
import random
from collections import OrderedDict

import numpy as np
import torch

from . import groundtruth, postprocess
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


# ---------------------------------------------------------------- UnrealStereo4kDataset
def _cfg_get(cfg, key):
    return cfg[key] if isinstance(cfg, dict) else getattr(cfg, key)


def rotate_matrix(angle, W, H):
    """the matrix Image.rotate(angle) of Pillow hands to its affine transform (output pixel centre -> source position), in Python floats
    exactly as PIL/Image.py builds it: angle % 360 first (it changes the last bits of sine and cosine for negative angles)"""
    angle = angle % 360.0
    if angle in (90.0, 180.0, 270.0):
        raise NotImplementedError("Image.rotate transposes at multiples of 90 degrees instead of resampling; not reproduced")
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = W / 2.0, H / 2.0
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def fix16(m):
    """the six 16.16 integers of Pillow's nearest-neighbour affine path (include/pf_hip.h, pf_aug_planes_nearest)"""
    def fix(v):
        return int(math.floor(v * 65536.0 + 0.5))
    return [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]


def draw_augmentation(degree, image_shape, crop_shape):
    """Every random number of one train sample, drawn on the host before anything is launched, from Python's `random` and `np.random` in
    the reference's order: aug_rotate (one random()), aug_color (one random(); above 0.5 also uniform(0.9, 1.1) for gamma, the same for
    brightness and np.random.uniform(0.9, 1.1, size=3)), aug_flip (one random()), random_crop (randint(0, H - h), randint(0, W - w)).
    -> (angle, colour = (gamma, brightness, colours) or None, flip, h0, w0)"""
    angle = (random.random() - 0.5) * 2 * degree
    colour = None
    if random.random() > 0.5:
        gamma = random.uniform(0.9, 1.1)
        brightness = random.uniform(0.9, 1.1)
        colour = (gamma, brightness, np.random.uniform(0.9, 1.1, size=3))
    flip = random.random() > 0.5
    h0 = random.randint(0, image_shape[0] - crop_shape[0])
    w0 = random.randint(0, image_shape[1] - crop_shape[1])
    return angle, colour, flip, h0, w0


METRIC_NAMES = ('a1', 'a2', 'a3', 'abs_rel', 'rmse', 'log_10', 'rmse_log', 'silog', 'sq_rel', 'see')     # u4k_dataset.py:200-209


class UnrealStereo4kDataset:
    def __init__(self, mode, data_root, split, transform_cfg, min_depth, max_depth, patch_raw_shape=(540, 960), resize_mode='zoe', *,
                 device="cuda", ops=None, image_shape=(2160, 3840)):
        self.dataset_name = 'u4k'
        self.mode = mode
        self.data_root = data_root
        self.split = split
        self.data_infos = self.load_data_list()
        self.min_depth = min_depth
        self.max_depth = max_depth
        if resize_mode == 'zoe':
            multiple = 32
        elif resize_mode == 'depth-anything':
            multiple = 14
        else:
            raise NotImplementedError
        self.patch_raw_shape = patch_raw_shape
        if isinstance(transform_cfg, dict):
            transform_cfg['random_crop_size'] = patch_raw_shape
        else:
            transform_cfg.random_crop_size = patch_raw_shape
        self.transform_cfg = transform_cfg
        self.image_shape = (int(image_shape[0]), int(image_shape[1]))        # the reference hard-codes 2160 x 3840
        self.device = torch.device(device)
        self.ops = ops
        self.process_shape = _network_shape(_cfg_get(transform_cfg, 'network_process_size'), multiple)
        self.preprocess = ImagePreprocessor(image_resolution=self.image_shape, process_shape=self.process_shape, dataset_name='u4k',
                                            device=self.device, ops=ops)
        self.timing = None          # a dict here receives the seconds per stage of __getitem__('train'), each ended by a synchronise

    def load_data_list(self):
        """u4k_dataset.py:58-107: four-column split lines, .png -> .raw, the depth factor from the two extrinsics files"""
        if self.split is None:
            raise NotImplementedError
        img_infos = []
        with open(self.split) as f:
            for line in f:
                img_l, _img_r, depth_map_l, _depth_map_r = line.strip().split(" ")
                img_l = img_l[:-3] + 'raw'
                info = dict(depth_map_path=os.path.join(self.data_root, depth_map_l), img_path=os.path.join(self.data_root, img_l),
                            filename=img_l, depth_fields=[])
                ext_name_l = info['depth_map_path'].replace('Disp0', 'Extrinsics0').replace('npy', 'txt')
                ext_name_r = info['depth_map_path'].replace('Disp0', 'Extrinsics1').replace('npy', 'txt')
                with open(ext_name_l, 'r') as g:
                    ext_l = g.readlines()
                with open(ext_name_r, 'r') as g:
                    ext_r = g.readlines()
                focal = float(ext_l[0].split(' ')[0])
                base = abs(float(ext_l[1].split(' ')[3]) - float(ext_r[1].split(' ')[3]))
                info['focal'] = focal
                info['depth_factor'] = base * focal
                img_infos.append(info)
        return sorted(img_infos, key=lambda x: x['img_path'])

    def __len__(self):
        return len(self.data_infos)

    def _raw_image(self, path):
        H, W = self.image_shape
        raw = np.fromfile(path, dtype=np.uint8)
        if raw.size != H * W * 3:
            raise ValueError(f"{path}: a 'u4k' image of {H} x {W} holds {H * W * 3} bytes, got {raw.size}")
        return raw.reshape(H, W, 3)

    def _tick(self, key, t0):
        if self.timing is None:
            return t0
        import time
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        now = time.perf_counter()
        self.timing[key] = self.timing.get(key, 0.0) + now - t0
        return now

    def __getitem__(self, idx):
        info = self.data_infos[idx]
        basename = os.path.splitext(info['filename'])[0].replace('/', '_')[1:]
        if self.mode != 'train':
            image = self.preprocess(self._raw_image(info['img_path']))
            gt = read_depth_gt(info['depth_map_path'], 'u4k', depth_factor=info['depth_factor'], device=self.device, ops=self.ops)
            return {'image_lr': image["image_lr"], 'image_hr': image["image_hr"], 'depth_gt': gt.depth.unsqueeze(0),
                    'boundary': gt.edge.unsqueeze(0), 'img_file_basename': basename}
        return self._train_sample(info, basename)

    def _train_sample(self, info, basename):
        import time
        ops, dev = groundtruth._ops(self.ops), self.device
        H, W = self.image_shape
        h, w = int(self.patch_raw_shape[0]), int(self.patch_raw_shape[1])
        angle, colour, flip, h0, w0 = draw_augmentation(_cfg_get(self.transform_cfg, 'degree'), (H, W), (h, w))   # before any launch
        matrix = rotate_matrix(angle, W, H)
        raw = self._raw_image(info['img_path'])
        with open(info['depth_map_path'], "rb") as f:
            payload = f.read()
        t0 = time.perf_counter()
        img_u8 = torch.from_numpy(raw).to(dev)
        box = torch.tensor([[w0, h0, w0 + w, h0 + h]], dtype=torch.int32).to(dev)
        bboxs = torch.tensor([w0, h0, w0 + w, h0 + h]).to(dev)
        image_hr = torch.tensor([H, W]).to(dev)                             # the reference returns the size here "to save some memory"
        t0 = self._tick("upload", t0)
        gt = read_depth_gt(payload, 'u4k', depth_factor=info['depth_factor'], device=dev, edges=False, ops=ops)
        if tuple(gt.depth.shape) != (H, W):
            raise ValueError(f"{info['depth_map_path']}: the disparity map is {tuple(gt.depth.shape)}, the image {H} x {W}")
        t0 = self._tick("ground_truth", t0)
        # the reference rotates, flips and crops the disparity plane as well and then drops it: only the depth plane is returned
        depth = ops.aug_planes_nearest([gt.depth], fix16(matrix), flip, [torch.empty((H, W), dtype=torch.float32, device=dev)])[0]
        crop_depths = depth[h0:h0 + h, w0:w0 + w].unsqueeze(0).contiguous()
        t0 = self._tick("planes", t0)
        image = ops.aug_image_u8_to_f32(img_u8, matrix, flip, colour, torch.empty((3, H, W), dtype=torch.float32, device=dev))
        t0 = self._tick("image", t0)
        image_lr = torch.empty((3,) + self.process_shape, dtype=torch.float32, device=dev)
        for c in range(3):
            ops.resize_bilinear_f32(image[c], image_lr[c])
        crops = torch.empty((1, 3) + self.process_shape, dtype=torch.float32, device=dev)
        ops.crop_resize(image, box, crops)
        self._tick("resizes", t0)
        return {'image_lr': image_lr, 'image_hr': image_hr, 'crops_image_hr': crops[0], 'depth_gt': depth.unsqueeze(0),
                'crop_depths': crop_depths, 'bboxs': bboxs, 'img_file_basename': basename}

    def get_metrics(self, depth_gt, result, disp_gt_edges, **kwargs):
        return postprocess.compute_metrics(depth_gt, result, disp_gt_edges=disp_gt_edges, min_depth_eval=self.min_depth,
                                           max_depth_eval=self.max_depth, garg_crop=False, eigen_crop=False, dataset='', ops=self.ops)

    def evaluator(self, capacity=64):
        """a DepthEvaluator with get_metrics' arguments: the same numbers without a host synchronisation per image"""
        return postprocess.DepthEvaluator(self.min_depth, self.max_depth, garg_crop=False, eigen_crop=False, dataset='', capacity=capacity,
                                          ops=self.ops)

    def pre_eval_to_metrics(self, pre_eval_results):
        """u4k_dataset.py:188-213: the per-image metric dicts, by position, to the nanmean of the ten metrics"""
        columns = tuple(zip(*[item.values() for item in pre_eval_results]))
        return {name: np.nanmean(columns[i]) for i, name in enumerate(METRIC_NAMES)}

    def evaluate(self, results, **kwargs):
        """u4k_dataset.py:215-259; the summary table is plain text"""
        ret_metrics = self.pre_eval_to_metrics(results)
        summary = OrderedDict((k, np.round(np.nanmean(v), 7)) for k, v in ret_metrics.items())
        cells = [(k, str(v)) for k, v in summary.items()]
        widths = [max(len(k), len(v)) for k, v in cells]
        rule = "+" + "+".join("-" * (n + 2) for n in widths) + "+"
        table = "\n".join([rule, "|" + "|".join(f" {k:^{n}} " for (k, _), n in zip(cells, widths)) + "|", rule,
                           "|" + "|".join(f" {v:^{n}} " for (_, v), n in zip(cells, widths)) + "|", rule])
        print('Evaluation Summary: \n' + table)
        return dict(ret_metrics)


def collate_train(samples):
    """a list of UnrealStereo4kDataset train samples -> the keyword arguments of PatchFusion(mode='train', ...): every tensor stacked
    along a new batch axis (the names stay behind)"""
    keys = ('image_lr', 'image_hr', 'depth_gt', 'crops_image_hr', 'crop_depths', 'bboxs')
    return {k: torch.stack([s[k] for s in samples]) for k in keys}

"""Whole frames for ``evaluate.py --full_frame``: the files ``AlignedDataset`` pairs (the sorted halves of
``dataroot/phase``), or the A half of ``dataroot`` as ``SingleDataset`` serves it (``--dataset_mode
single``), each decoded to one uint8 [H, W, 3] array and served as it is.

No crop, no flip and no RNG draw; a directory may hold frames of different sizes, so the loader hands out
one frame per item and never stacks them.  A frame smaller than the tile is refused by file name."""
import os

import numpy as np
import torch
from PIL import Image

from data.image_folder import make_dataset


class FrameDataset(torch.utils.data.Dataset):
    def initialize(self, opt):
        self.opt = opt
        self.single = opt.dataset_mode == "single"
        if self.single:
            self.A_paths, self.B_paths = sorted(make_dataset(opt.dataroot)[0]), None
        elif opt.dataset_mode == "aligned":
            self.A_paths, self.B_paths = sorted(make_dataset(os.path.join(opt.dataroot, opt.phase)))
        else:
            raise ValueError("Dataset [%s] not recognized." % opt.dataset_mode)

    def _frame(self, path):
        img = np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)
        th, tw = self.opt.fineSize_h, self.opt.fineSize_w
        if img.shape[0] < th or img.shape[1] < tw:
            raise ValueError("FrameDataset: %s is %dx%d, smaller than the %dx%d tile (padding is not supported)"
                             % (path, img.shape[0], img.shape[1], th, tw))
        return torch.from_numpy(img.copy())

    def __getitem__(self, index):
        item = {"A_u8": self._frame(self.A_paths[index]), "A_paths": self.A_paths[index]}
        if not self.single:
            item["B_u8"] = self._frame(self.B_paths[index])
            item["B_paths"] = self.B_paths[index]
            if item["B_u8"].shape != item["A_u8"].shape:
                raise ValueError("FrameDataset: %s is %dx%d but its pair %s is %dx%d"
                                 % ((self.A_paths[index],) + tuple(item["A_u8"].shape[:2])
                                    + (self.B_paths[index],) + tuple(item["B_u8"].shape[:2])))
        return item

    def __len__(self):
        return len(self.A_paths)

    def name(self):
        return "FrameDataset"


def frame_loader(opt):
    """Frames in order, one per item (``batch_size=None``: no stacking), decoded by ``--nThreads`` workers."""
    dataset = FrameDataset()
    dataset.initialize(opt)
    print("dataset [%s] was created" % dataset.name())
    return torch.utils.data.DataLoader(dataset, batch_size=None, shuffle=False, num_workers=int(opt.nThreads))

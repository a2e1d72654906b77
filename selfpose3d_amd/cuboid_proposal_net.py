"""Root-localisation net: unproject (coarse grid) -> V2V -> NMS/top-k proposals.

Interface of /root/reference/lib/models/cuboid_proposal_net.py:86-122 (``CuboidProposalNet``)
and :13-83 (``ProposalLayer``); checkpoint keys ``v2v_net.*`` are identical.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from .project_layer import ProjectLayer
from .proposal import nms_with_locations
from .v2v_net import TiledZSpectrum, V2VNet


class ProposalLayer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.grid_size = [float(v) for v in cfg.MULTI_PERSON.SPACE_SIZE]
        self.cube_size = [int(v) for v in cfg.MULTI_PERSON.INITIAL_CUBE_SIZE]
        self.grid_center = [float(v) for v in cfg.MULTI_PERSON.SPACE_CENTER]
        self.num_cand = int(cfg.MULTI_PERSON.MAX_PEOPLE_NUM)
        self.threshold = float(cfg.MULTI_PERSON.THRESHOLD)

    @staticmethod
    def match_to_gt(locs, gt_3d, num_person):
        """index of the nearest GT root within 500 mm, else -1 (cuboid_proposal_net.py:25-40), batched."""
        B, K, _ = locs.shape
        P = gt_3d.shape[1]
        d = torch.sqrt(((locs[:, :, None, :] - gt_3d[:, None, :, :]) ** 2).sum(-1))      # (B,K,P)
        live = torch.arange(P, device=locs.device)[None, None, :] < num_person.to(locs.device).view(B, 1, 1)
        d = torch.where(live, d, torch.full_like(d, float("inf")))
        min_dist, min_gt = d.min(dim=-1)
        out = min_gt.float()
        out[min_dist > 500.0] = -1.0
        return out

    def forward(self, root_cubes, meta):
        B = root_cubes.shape[0]
        if root_cubes.is_cuda and not (self.training and ("roots_3d" in meta[0] and "num_person" in meta[0])):
            # eval: [x,y,z, (score > THRESHOLD) - 1, score] straight from the NMS merge kernel
            from . import _lib
            return _lib.nms_proposals(root_cubes.detach(), self.num_cand, self.grid_size, self.grid_center, self.threshold)
        vals, _idx, locs = nms_with_locations(root_cubes, self.num_cand, self.grid_size, self.grid_center)
        grid_centers = torch.zeros(B, self.num_cand, 5, device=root_cubes.device)
        grid_centers[:, :, 0:3] = locs
        grid_centers[:, :, 4] = vals
        if self.training and ("roots_3d" in meta[0] and "num_person" in meta[0]):
            gt = meta[0]["roots_3d"].float().to(root_cubes.device)
            grid_centers[:, :, 3] = self.match_to_gt(locs, gt, meta[0]["num_person"])
        else:
            grid_centers[:, :, 3] = (vals > self.threshold).float() - 1.0
        return grid_centers


class Front(NamedTuple):
    """the call a net makes for its V2V input: ``get_voxel_zspectrum(..., SZ=sz)`` -> ``TiledZSpectrum`` when ``sz`` is set, else
    ``get_voxel(..., want_grids=False, pad_channels, channels_last)`` - with ``out``, into the opening conv's input view"""
    sz: Optional[int]
    pad_channels: bool
    channels_last: bool
    out: bool


def front_rule(net, hms, fronts=()) -> Front:
    """How ``net`` (``project_layer``, ``v2v_net``, ``cube_size``, ``channels_last``; ``rootnet_roothm`` where it has one) takes
    the heat-map list ``hms`` to its V2V net.  ``fronts``: the fused z-spectrum fronts this caller takes - "zdft" (13..16
    joints; and, where the spectrum is not wanted, channels-last 16-channel cubes for the HIP z pass), "wide" (17..32,
    SP3D_WIDE_FRONT=1), "one" (the one channel of ROOTNET_ROOTHM, SP3D_ONE_FRONT=1).  Whether the layer delivers a front is
    ``ProjectLayer.spectrum_route``'s answer and whether the opening conv starts from it ``V2VNet.wants_zspectrum``'s, so
    the nets and the layer cannot disagree; ``out`` is ``ProjectLayer.takes_out``'s."""
    pl, v2v = net.project_layer, net.v2v_net
    planar = v2v.wants_planar_input() and hms[0].is_cuda      # FFT opening conv (inference, no grad): plain J-channel cubes
    direct = planar and pl.takes_out(hms)                      # ... which the kernel writes into that conv's padded input buffer
    route = pl.spectrum_route(hms) if direct and fronts else None
    if route is not None:
        # ... or not at all: the kernel emits the z-spectrum of the cubes, which is what the opening conv computes first
        front = "one" if route.read == "one" else ("wide" if route.jp == 32 else "zdft")
        if front in fronts and (front != "one" or getattr(net, "rootnet_roothm", False)):
            sz = v2v.wants_zspectrum(*net.cube_size, hms[0].shape[1])
            if sz is not None:
                return Front(sz, False, False, False)
    cl16 = direct and "zdft" in fronts and v2v.wants_channels_last_cubes(*net.cube_size)
    return Front(None, cl16 or not planar, cl16 or (net.channels_last and not planar), direct and not cl16)


class CuboidProposalNet(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.grid_size = [float(v) for v in cfg.MULTI_PERSON.SPACE_SIZE]
        self.cube_size = [int(v) for v in cfg.MULTI_PERSON.INITIAL_CUBE_SIZE]
        self.grid_center = [float(v) for v in cfg.MULTI_PERSON.SPACE_CENTER]
        self.rootnet_roothm = bool(cfg.NETWORK.ROOTNET_ROOTHM)
        self.root_id = cfg.DATASET.ROOTIDX_PSEUDO
        self.project_layer = ProjectLayer(cfg)
        self.v2v_net = V2VNet(1 if self.rootnet_roothm else int(cfg.NETWORK.NUM_JOINTS), 1)
        self.proposal_layer = ProposalLayer(cfg)
        self.channels_last = False      # set by use_channels_last()

    def use_channels_last(self, on: bool = True):
        """run the V2V stack in torch.channels_last_3d (MIOpen NDHWC kernels, no internal transposes)"""
        self.channels_last = bool(on)
        self.v2v_net.to(memory_format=torch.channels_last_3d if on else torch.contiguous_format)
        return self

    def use_bf16_heatmaps(self, on: bool = True):
        """read the heat-maps as bf16 and keep every result fp32 (``ProjectLayer.bf16_maps``); no effect under autograd"""
        self.project_layer.bf16_maps = bool(on)
        return self

    def use_bf16_training(self, on: bool = True):
        """train through bf16 heat-maps: maps that are bf16 and carry a gradient are read as bf16 by the masked training
        forwards, every result stays fp32 and the gradient leaves as bf16 (``ProjectLayer.bf16_train``); fp32 maps and
        inference are untouched"""
        self.project_layer.bf16_train = bool(on)
        return self

    def forward(self, all_heatmaps, meta, flip_xcoords=None):
        if self.rootnet_roothm:                                   # root-joint channel only (:103-108)
            hms = [a[:, self.root_id:self.root_id + 1] for a in all_heatmaps]      # a view: read in place with ProjectLayer.one_channel, copied otherwise
        else:
            hms = all_heatmaps
        front = front_rule(self, hms, fronts=("zdft", "wide", "one"))
        if front.sz is not None:
            spec = self.project_layer.get_voxel_zspectrum(hms, meta, self.grid_size, [self.grid_center], self.cube_size, front.sz,
                                                          flip_xcoords=flip_xcoords)
            root_cubes = self.v2v_net(TiledZSpectrum(spec, *self.cube_size, front.sz)).squeeze(1)
            return root_cubes, self.proposal_layer(root_cubes, meta)
        out = self.v2v_net.input_view(hms[0].shape[0], *self.cube_size, hms[0].device) if front.out else None
        cubes, _ = self.project_layer.get_voxel(hms, meta, self.grid_size, [self.grid_center], self.cube_size,
                                                flip_xcoords=flip_xcoords, want_grids=False, pad_channels=front.pad_channels,
                                                channels_last=front.channels_last, out=out)
        root_cubes = self.v2v_net(cubes).squeeze(1)
        return root_cubes, self.proposal_layer(root_cubes, meta)

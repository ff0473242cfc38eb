"""A stand-in for the object dropin.fast_forward_perpix is bound to, for tests that must run where the reference's Python tree is
absent: a plain attribute holder with exactly what GeneratorBinding.why_not_perpix / sync / rays and fast_forward_perpix read --
the three networks and the hash grid as this package's own modules with the synthetic weights, the inference flags, the label
table, the scene volume -- and a `_forward_perpix_reference` that raises, so that a call which leaves the native routes is seen.
It is not a generator: it has no forward, no frame loop and no voxlib."""
import json
import os
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class ReferenceMethodCalled(RuntimeError):
    """The call was handed to _forward_perpix_reference (which this holder does not have)."""


def _load(module, weights, prefix):
    module.load_state_dict({k[len(prefix):]: torch.as_tensor(np.asarray(v)) for k, v in weights.items() if k.startswith(prefix)})
    module = module.cuda().eval()
    for p in module.parameters():
        p.requires_grad_(False)
    return module


class PerpixHost:
    def __init__(self, weights, scene, num_samples):
        from scenedreamer_amd import dropin, modules
        from scenedreamer_amd.gridencoder import GridEncoder
        self.render_net = _load(modules.LightningMLP(128, 256, 0, mask_dim=12, out_channels_s=1, out_channels_c=64), weights, "render_net.")
        self.sky_net = _load(modules.SKYMLP(33, 256, 64), weights, "sky_net.")
        self.denoiser = _load(modules.RenderCNN(64, 256), weights, "denoiser.")
        self.hash_encoder = _load(GridEncoder(input_dim=5, num_levels=16, level_dim=8, base_resolution=16, log2_hashmap_size=19,
                                              desired_resolution=2048), weights, "hash_encoder.")
        # the flags inference_givenstyle runs with (scenedreamer.py:547-555 over the shipped inference config)
        self.num_samples = int(num_samples)
        self.num_blocks_early_stop = 6
        self.sample_depth = 3
        self.dists_scale = 0.25
        self.coarse_deterministic_sampling = True
        self.sample_use_box_boundaries = False
        self.raw_noise_std = 0.0
        self.keep_sky_out = True
        self.keep_sky_out_avgpool = True
        self.sky_global_avgpool = True
        self.clip_feat_map = True
        self.pe_params = [0, 0, 0, False]
        self.pe_params_sky = [5, True]
        lt = json.load(open(os.path.join(ROOT, "scenedreamer_amd", "data", "mc2reduced.json")))
        self.label_trans = types.SimpleNamespace(mcid2rdid_lut=torch.tensor(lt["lut"], dtype=torch.long), ignore_id=int(lt["ignore_id"]),
                                                 dirt_id=int(lt["dirt_id"]))
        self.voxel = types.SimpleNamespace(voxel_t=scene.voxel_t.cuda())
        self._forward_perpix = types.MethodType(dropin.fast_forward_perpix, self)

    def _forward_perpix_reference(self, *args, **kwargs):
        raise ReferenceMethodCalled("the call left the native routes")

"""Generate tests/golden/plugin_seam.json from the REFERENCE (build container only).

    python oracle/make_golden_seam.py <reference checkout>

Records what tests/test_host_logic.py::test_plugin_seam_matches_the_recorded_reference compares the HIP classes with:
  * the `unet_config`, `first_stage_config` and `cond_stage_config` nodes of the reference's
    `configs/stable-diffusion/v1-inference.yaml` (parsed: targets and hyper-parameters);
  * the state_dict keys / shapes of the reference's own `UNetModel` and `AutoencoderKL` (its `loss.*` entries excluded),
    built by the reference's `instantiate_from_config` (ldm/util.py:78-93) from those nodes on the meta device.
The GPU box has no reference checkout: the test reads the fixture only.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).
"""
import contextlib
import io
import json
import os
import sys

import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(ref):
    sys.path.insert(0, ref)
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import run_reference_script as launcher
    launcher.install_stubs(have_gpu=True, offline_stubs=True)   # pytorch_lightning / taming stand-ins for AutoencoderKL's imports
    from ldm.util import instantiate_from_config
    with open(os.path.join(ref, 'configs', 'stable-diffusion', 'v1-inference.yaml')) as f:
        params = yaml.safe_load(f)['model']['params']
    doc = {'source': 'configs/stable-diffusion/v1-inference.yaml and ldm.util.instantiate_from_config of the reference '
                     '(meta device); written by oracle/make_golden_seam.py'}
    for node in ('unet_config', 'first_stage_config', 'cond_stage_config'):
        doc[node] = params[node]
    with torch.device('meta'), contextlib.redirect_stdout(io.StringIO()):
        unet = instantiate_from_config(params['unet_config'])
        vae = instantiate_from_config(params['first_stage_config'])
    doc['unet_state'] = {k: list(v.shape) for k, v in unet.state_dict().items()}
    doc['first_stage_state'] = {k: list(v.shape) for k, v in vae.state_dict().items() if not k.startswith('loss.')}
    out = os.path.join(ROOT, 'tests', 'golden', 'plugin_seam.json')
    with open(out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print(f'{out}: {len(doc["unet_state"])} UNet tensors, {len(doc["first_stage_state"])} first-stage tensors')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])

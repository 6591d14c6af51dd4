"""Golden data for the config surface (build container only; test infrastructure).

    python -m oracle.ref_harness.make_config_golden REFERENCE_ROOT     # writes tests/golden/config_reference_options.json

`config_reference_options.json`: what nuhtc_amd.config.engine_options reads off the reference's own PanNuke config file
(configs/nuhtc/htc_lite_swin_pytorch_fpn_PanNuke_seasaw_CAS.py of the reference tree, loaded unchanged by Config.fromfile).
tests/test_host.py checks the project's own config against it.
"""
import json
import os
import sys

OUT = os.path.join(os.path.dirname(__file__), '..', '..', 'tests', 'golden')
CFG = 'configs/nuhtc/htc_lite_swin_pytorch_fpn_PanNuke_seasaw_CAS.py'


def main(ref):
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', '..'))
    from nuhtc_amd.config import Config, engine_options
    o = engine_options(Config.fromfile(os.path.join(ref, CFG)))
    with open(os.path.join(OUT, 'config_reference_options.json'), 'w') as f:
        json.dump(dict(source=CFG, engine_options=o), f, indent=1)
        f.write('\n')
    print(json.dumps(o))


if __name__ == '__main__':
    main(sys.argv[1])

"""Device-side training input pipeline: the MI355X counterpart of the reference's per-sample host transforms
Compose([Resize(256), RandomScaleCrop(256), Normalize_tf(), ToTensor()]) (train.py:58-62; custom_transforms.py:375-391,
330-354,139-176,455-499,581-599) and of get_multi_batch's stack + .cuda() (Trainer.py:45-55).

The decoded uint8 samples are copied to the GPU as they are; resampling, cropping, normalisation and the mask thresholds run
there (csrc/pipeline.hip) and produce the [N,3,S,S] / [N,1,S,S] fp32 batch the training step takes.  The result equals the
reference's bit for bit (tests/test_input_pipeline_gpu.py, fixtures generated from the reference's own classes).

What stays on the host: PNG decoding and the random draws.

One module per subject.  The host specifications import numpy only: `resample` (Pillow's coefficient tables and the crop's draws),
`augment` (the reference's six training augmentations), and one per optional stage behind the augmentations — `amplitude_mix`,
`appearance`, `quality`, `jpeg`, `clahe` — each with its config class, its draws, its parameter check and its numpy specification.
`stages` ties those five to one protocol and holds the two orders (run and draw); `pipeline` is the device pipeline.  Every name
is re-exported here: `from wtpse_hip.input_pipeline import X` is how the rest of the project reads them.
"""
from .resample import PRECISION_BITS, draw, nearest_table, resample_table
from .augment import Augment, augment_host, draw_augment, elastic_displacement, gamma_table, gaussian_weights
from .amplitude_mix import MIX_SIZES, AmplitudeMix, _check_mix_size, amplitude_mix_host, check_mix_params, draw_mix, twiddle_table
from .appearance import (APPEARANCE_B_OFF, APPEARANCE_BIAS_MAX, APPEARANCE_BLEND, APPEARANCE_CHANNELS, APPEARANCE_CL, APPEARANCE_COLS,
                         APPEARANCE_LAYERS, APPEARANCE_MAX_SIZE, APPEARANCE_NET_COLS, APPEARANCE_R_MAX, APPEARANCE_SELECTED,
                         APPEARANCE_SPACING, APPEARANCE_W_MAX, APPEARANCE_W_OFF, AppearanceNets, _check_appearance_size,
                         appearance_axis_table, appearance_field_host, appearance_gain, appearance_grid, appearance_host,
                         appearance_is_neutral, appearance_layer_host, appearance_net_of, appearance_net_row, appearance_neutral,
                         check_appearance_params, draw_appearance)
from .quality import (QUALITY_A, QUALITY_BETA, QUALITY_C, QUALITY_COLS, QUALITY_K, QUALITY_MAX_SIZE, QUALITY_RADIUS, ImageQuality,
                      _check_quality_size, check_quality_params, draw_quality, quality_host, quality_is_neutral, quality_neutral,
                      quality_noise_host, quality_positions, quality_taps)
from .jpeg import (JPEG_IDCT_WINDOW, JPEG_MAX_SIZE, JpegCompression, _check_jpeg_size, check_jpeg_params, draw_jpeg, jpeg_host,
                   jpeg_is_neutral, jpeg_neutral, jpeg_reciprocals, jpeg_tables)
from .clahe import (CLAHE_MAX_SIDE, CLAHE_MAX_TILES, CLAHE_MODES, Clahe, check_clahe, clahe_axis_table, clahe_bounds,
                    clahe_device_tables, clahe_host, clahe_lut, clahe_luts_host, clahe_record, clahe_redistribute, parse_clahe)
from .stages import DRAW_ORDER, RUN_ORDER, Stage
from .pipeline import DeviceInputPipeline, _dev_i32, _dev_u8, device_uniform

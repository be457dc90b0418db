"""The optional stages behind the crop / augmentation step, under one protocol, and the two orders they stand in.

A `Stage` carries
    feed_kw     the keyword that hands its config to `trainer.FundusBatches` (None there: the stage is off)
    pipe_kw     the keyword that hands its value for one batch to `DeviceInputPipeline.__call__` (None there: off)
    config      the type of that config
    check_size(S, config)     ValueError unless the stage takes samples of side S
    draw(np_rng, n, feed)     the value for a batch of n samples, drawn from the run's numpy generator
    check(value, N, S)        the value after the checks the device arithmetic rests on (ValueError otherwise)
    idle(value)               True when the whole batch is neutral: nothing is launched
    run(pipe, img, value)     the uint8 batch [N,S,S,3] after the stage (through `ops`, looked up at call time)
A stage that is off adds nothing: no draw, no check, no launch, no allocation.  A new stage is its module here, its kernel file,
its `ops` wrapper and one entry in each of the two tuples at the end.
"""
from collections import namedtuple

import numpy as np

from .. import ops
from .amplitude_mix import AmplitudeMix, _check_mix_size, check_mix_params, draw_mix
from .appearance import AppearanceNets, _check_appearance_size, appearance_is_neutral, check_appearance_params, draw_appearance
from .clahe import Clahe, check_clahe
from .jpeg import JpegCompression, _check_jpeg_size, check_jpeg_params, draw_jpeg, jpeg_is_neutral
from .quality import ImageQuality, _check_quality_size, check_quality_params, draw_quality, quality_is_neutral

Stage = namedtuple("Stage", "feed_kw pipe_kw config check_size draw check idle run")


def _draw_mix(np_rng, n, feed):
    partner, lam = draw_mix(np_rng, len(feed.datasets), feed.per_domain, feed.style)
    return partner, lam, feed.style.band(feed.size)


def _check_jpeg(value, N, S):
    _check_jpeg_size(S)
    return check_jpeg_params(value[0], value[1], N)


def _run_quality(pipe, img, params):
    # (the seed as the C ABI sees it: ctypes reduces wtpse_uniform_f64's modulo 2^64 too)
    img, pipe.quality_pos = ops.image_quality(img, params, pipe.noise_seed & ((1 << 64) - 1), pipe.quality_pos, want_pos=True)
    return img


# value = (partner, lam, b): `draw_mix`'s two arrays and `AmplitudeMix.band(size)`.  Needs at least two source domains in a batch.
mix = Stage("style", "mix_draws", AmplitudeMix,
            check_size=lambda S, config: _check_mix_size(S),
            draw=_draw_mix,
            check=lambda value, N, S: check_mix_params(*value, N, S),
            idle=lambda value: not np.any(np.asarray(value[0]) >= 0),
            run=lambda pipe, img, value: ops.amplitude_mix(img, *value))

# value = (params, field, spacing): `draw_appearance`'s two arrays and `AppearanceNets.spacing`.  Reads no device random stream.
appearance = Stage("appearance", "appearance_draws", AppearanceNets,
                   check_size=lambda S, config: _check_appearance_size(S, config.spacing),
                   draw=lambda np_rng, n, feed: draw_appearance(np_rng, n, feed.size, feed.appearance) + (feed.appearance.spacing,),
                   check=lambda value, N, S: check_appearance_params(value[0], value[1], N, S, value[2]) + (value[2],),
                   idle=lambda value: appearance_is_neutral(value[0]).all(),
                   run=lambda pipe, img, value: ops.appearance_nets(img, *value))

# value = `draw_quality`'s parameter table [N,13].  Its noise comes from the device Philox stream `pipe.noise_seed` — blocks of
# their own, which no other consumer of the seed reads — at the running position `pipe.quality_pos` (S * S positions per sample
# with k > 0, in batch order): run state, like `pipe.noise_pos`.
quality = Stage("quality", "quality_draws", ImageQuality,
                check_size=lambda S, config: _check_quality_size(S),
                draw=lambda np_rng, n, feed: draw_quality(np_rng, n, feed.quality),
                check=lambda value, N, S: check_quality_params(value, N),
                idle=lambda value: quality_is_neutral(value).all(),
                run=_run_quality)

# value = `draw_jpeg`'s (mode [N], tables [N,2,64]).  The side must be a multiple of 16.  Reads no device random stream.
jpeg = Stage("jpeg", "jpeg_draws", JpegCompression,
             check_size=lambda S, config: _check_jpeg_size(S),
             draw=lambda np_rng, n, feed: draw_jpeg(np_rng, n, feed.jpeg),
             check=_check_jpeg,
             idle=lambda value: jpeg_is_neutral(value[0]).all(),
             run=lambda pipe, img, value: ops.jpeg_roundtrip(img, *value))

# value = the `Clahe` itself: preprocessing, not an augmentation — it draws nothing and is never idle.
clahe = Stage("clahe", "clahe", Clahe,
              check_size=lambda S, config: config.check_size(S, S),
              draw=lambda np_rng, n, feed: feed.clahe,
              check=lambda value, N, S: check_clahe(value, S, S),
              idle=lambda value: False,
              run=lambda pipe, img, value: ops.clahe(img, value))

# The order the stages run in, on the uint8 batch between the crop / augmentation step and the normalisation: appearance changes
# first (another domain's amplitudes, then a random remapping), then the camera is simulated (optics and sensor, then the file it
# writes), then the preprocessing reads that file.
RUN_ORDER = (mix, appearance, quality, jpeg, clahe)

# The order the stages draw in from the run's numpy generator, after all of a batch's other draws.  It is the order in which the
# stages were ADDED to the project, not the run order: a new stage is appended here, never inserted, because every stage in
# front of it then draws exactly what it drew before the new one existed — a seeded run keeps its stream whatever is switched on
# behind it.
DRAW_ORDER = (mix, quality, clahe, appearance, jpeg)

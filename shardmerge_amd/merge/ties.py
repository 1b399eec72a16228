"""TiesMerge: TIES-Merging (Yadav et al., 2023) - trim each finetune's delta to its largest entries, elect a sign
per parameter by the weighted sum, merge the agreeing entries, add the result onto output_base_model.  The reference
has no such operator; the function is defined in include/shardmerge_hip.h (``smhip_ties_merge``) and runs in three
HIP kernels (csrc/sm_ties.hpp) behind ``Engine.ties_merge``.

Tensor routing is FourierMerge's: embeddings / final norm / head pass through from the ``is_input`` / ``is_output``
finetune, every block tensor is merged over the finetunes whose layer window covers it, each against its own base.
Only the block-tensor merge (``merge_block``) differs, and there is no shape pre-flight: a streaming operator
takes every shape and rank."""
from __future__ import annotations

import logging
import math

from ..config import TIES_OPTION_DEFAULTS
from .base import MergeTensorsBase
from .fast_fourier import FourierMerge

logger = logging.getLogger(__name__)


class TiesMerge(FourierMerge):
    """Also the base of the other delta-merge operators (dare.py, breadcrumbs.py): they name their option_defaults and
    tensor_passes and state their own readme method line, merge_block and log line."""
    option_defaults = TIES_OPTION_DEFAULTS

    def __init__(self, config, index_manager=None, engine=None, **kwargs):
        for key, value in {**TIES_OPTION_DEFAULTS, **self.option_defaults}.items():
            setattr(self, key, value)
        super().__init__(config, index_manager=index_manager, engine=engine, **kwargs)     # (sets the YAML overrides, as floats)

    async def initialize(self):
        await MergeTensorsBase.initialize(self)          # no transform lengths to check

    def _readme(self, title: str, method: str) -> str:
        models = "\n".join(f"- {m.model} (vs {m.base}, weight {m.alpha})" for m in self.config.finetune_merge)
        return f"# {title} Merged Model\nBase: {self.config.output_base_model}\nMethod: {method}\nModels merged:\n{models}\n"

    def _how_and_norm(self, normalize):
        """the readme's words for sign_election and a normalize option (operators with the two modes)"""
        how = "elect sign, merge the agreeing entries" if self.sign_election else "add the weighted deltas"
        norm = ("normalized by the agreeing weights" if self.sign_election else "normalized by the sum of the weights") \
            if normalize else "plain sum"
        return how, norm

    def get_readme(self) -> str:
        return self._readme("TIES", f"TIES (trim, elect sign, merge), density {self.density:g}, lambda {self.ties_lambda:g}, "
                                    f"{'normalized by the agreeing weights' if self.ties_normalize else 'plain sum'}")

    def merge_block(self, eng, fts, bases, alphas, base_out, name: str):
        return eng.ties_merge(fts, bases, alphas, base_out, density=self.density, lam=self.ties_lambda,
                              normalize=bool(self.ties_normalize), layer_name=name)

    def tensor_passes(self, k: int) -> int:
        return 2 * k + 3

    def block_cost_ms(self, shape, k: int) -> float:
        """the partitioned path's cost model: tensor_passes(k) streaming passes over the tensor"""
        return 0.02 + 2.0 * math.prod(int(d) for d in shape) * self.tensor_passes(k) / 4.0e9

    def _log_block(self, name: str, k: int, report):
        logger.info(f"Merged {name}: {k} model(s), TIES kept {report.kept} of {report.k_keep} asked, thresholds "
                    f"{[float(f'{t:.4g}') for t in report.thresholds]}")

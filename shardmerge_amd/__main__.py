"""`python -m shardmerge_amd merge CONFIG` (and `python -m shard merge CONFIG`
through the alias package): the merge entry point of the reference CLI
(shard/__main__.py:78-158) with the same arguments and options; and `analyze CONFIG`,
the per-tensor task-vector statistics of the same config (merge/analyze.py), which
writes no tensor; and `extract-lora MODEL --base BASE --rank R --out DIR`, a PEFT LoRA adapter
from a full finetune (merge/extract.py); and `compress-delta MODEL --base BASE --out DIR`, a 1- or 2-bit delta
pack from a full finetune (merge/compress.py)."""
from __future__ import annotations

import asyncio
import logging
import traceback
from pathlib import Path
from typing import Optional

import click

from .config import MergeConfig
from .index import LocalModelIndex
from .merge.fast_fourier import FourierMerge

logger = logging.getLogger(__name__)


def setup_logging(verbose: bool):
    logging.basicConfig(level=logging.DEBUG if verbose else logging.INFO,
                        format="%(asctime)s - %(name)s - %(levelname)s - %(message)s")


async def run_merge(config: MergeConfig, device: str, clean_cache: bool, emr_pack_options=None, **kwargs):
    """Build the index and the operator, run the merge (reference __main__.py:47-76).
    With more than one rank (torchrun) the tensor list is partitioned over the GPUs.
    emr_pack_options (merge/emr_packs.py): the merge also writes every entry's EMR pack; what they rule out is rejected
    here, before an index is built or a path is chosen."""
    from . import distributed
    import os
    if emr_pack_options is not None:
        emr_pack_options.check(config)
        if emr_pack_options.asked:
            from .merge.emr_packs import EmrPackMerge
            index_manager = LocalModelIndex(storage_path=config.storage_path, cache_path=config.cache_path)
            await EmrPackMerge(config=config, index_manager=index_manager, emr_pack_options=emr_pack_options, **kwargs).merge(device=device)
            return
    index_manager = LocalModelIndex(storage_path=config.storage_path, cache_path=config.cache_path)
    # SHARDMERGE_INPLACE=1: a single process takes the multi-GPU path's in-place output shards too (pre-sized files,
    # every tensor pwritten at its offset as soon as its copy to the host is done) instead of writing a shard when it
    # is complete - one file takes ~7 GB/s on tmpfs whatever the thread count, so the sooner its writes start the better
    # (tools/cli_bench.py: 5.1 against 3.9 GB/s of merged weights on the Llama-3-70B slice)
    if distributed.world_size() > 1 or os.environ.get("SHARDMERGE_FORCE_DIST") == "1" or os.environ.get("SHARDMERGE_INPLACE") == "1":
        await distributed.run_partitioned_merge(config, index_manager, device)
        return
    from .merge import operator_class
    merger = operator_class(config.operator)(config=config, index_manager=index_manager, **kwargs)
    await merger.merge(device=device)


@click.group()
def cli():
    """Shard merge utility (MI355X-native merge path)."""


@cli.command("merge")
@click.argument("config_file", type=click.Path(exists=True, path_type=Path))
@click.option("--cache-dir", type=click.Path(path_type=Path), default=None, help="Directory for caching downloaded files")
@click.option("--clean_cache", is_flag=True, help="Delete cached files after merging")
@click.option("--device", type=str, default=None, help="Device to perform tensor operations on (cuda/cpu)")
@click.option("--verbose", is_flag=True, help="Enable verbose logging")
@click.option("--emr-packs", "emr_packs", type=click.Path(path_type=Path), default=None,
              help="operator emr: also write every entry's EMR pack, to DIR/<its model URI>-emr")
@click.option("--emr-unified", "emr_unified", type=str, default=None,
              help="With --emr-packs: the name under storage_dir at which the merged model will be found (recorded in every pack)")
@click.option("--emr-scale", "emr_scale", type=click.Choice(["model", "tensor"]), default=None,
              help="With --emr-packs: one rescaler for the whole model (default), or one per tensor")
@click.option("--emr-full", "emr_full", type=str, default=None,
              help="With --emr-packs: store whole the tensors whose name ends in one of these, comma-separated")
def merge_command(config_file: Path, cache_dir: Optional[Path], verbose: bool, emr_packs: Optional[Path], emr_unified: Optional[str],
                  emr_scale: Optional[str], emr_full: Optional[str], **kwargs):
    """Merge multiple finetuned models by computing and combining their deltas.

    CONFIG_FILE is a YAML file with output_base_model, finetune_merge (list of
    {model, base, alpha, is_input, is_output, start_layer, end_layer}) and output_dir.
    With operator emr, --emr-packs DIR --emr-unified NAME also writes what `emr-task` would write per entry afterwards.
    """
    setup_logging(verbose)
    from .constants import tune_hip_queues
    tune_hip_queues()                   # before the first GPU call (8 engines, 8 side streams)
    try:
        config = MergeConfig.from_yaml(config_file)
        logger.info(f"Loaded configuration: {config}")
        if cache_dir:
            config.cache_dir = cache_dir
        config.update({k: v for k, v in kwargs.items() if v is not None})
        from .merge.emr_packs import EmrPackOptions
        options = EmrPackOptions(emr_packs, emr_unified, emr_scale, emr_full)
        asyncio.run(run_merge(config=config, emr_pack_options=options, **config.to_dict()))
    except Exception as exc:
        logging.error(f"Error during merge: {exc}", exc_info=verbose)
        traceback.print_exc()
        raise click.Abort()


def _densities_option(ctx, param, value):
    from .merge.analyze import parse_densities
    try:
        return parse_densities(value)
    except ValueError as exc:
        raise click.BadParameter(str(exc))


@cli.command("analyze")
@click.argument("config_file", type=click.Path(exists=True, path_type=Path))
@click.option("--densities", default="0.05,0.1,0.2,0.5", callback=_densities_option,
              help="Up to four candidate densities in (0, 1], comma-separated")
@click.option("--report", type=click.Path(path_type=Path), default=None, help="Where the JSON goes (default: <output_dir>/analysis.json)")
@click.option("--device", type=str, default=None, help="Device to perform tensor operations on (cuda/cpu)")
@click.option("--verbose", is_flag=True, help="Enable verbose logging")
def analyze_command(config_file: Path, densities, report: Optional[Path], device: Optional[str], verbose: bool):
    """Task-vector statistics of every block tensor a merge of CONFIG_FILE would touch, no tensor written.

    Per finetune: norm, cosines, and at each candidate density what a trim keeps (elements, energy), how the kept sets
    overlap and what the TIES sign election would discard.  The full per-tensor report goes to a JSON file.
    """
    setup_logging(verbose)
    from . import distributed
    if distributed.world_size() > 1:
        raise click.ClickException("analyze runs in a single process: a partitioned analysis is not supported (run it without torchrun)")
    from .constants import tune_hip_queues
    tune_hip_queues()                   # before the first GPU call, as merge does
    try:
        config = MergeConfig.from_yaml(config_file)
        if device is not None:
            config.device = device
        from .merge.analyze import format_tables, run_analysis
        path = report if report is not None else config.output_path / "analysis.json"
        result = asyncio.run(run_analysis(config, config.device, densities, path))
    except click.ClickException:
        raise
    except Exception as exc:
        logging.error(f"Error during analyze: {exc}", exc_info=verbose)
        traceback.print_exc()
        raise click.Abort()
    click.echo(format_tables(result))
    click.echo(f"report: {path}")


@cli.command("extract-lora")
@click.argument("model", type=str)
@click.option("--base", required=True, type=str, help="The base model MODEL was finetuned from (under the storage directory)")
@click.option("--rank", required=True, type=int, help="The adapter's rank r, 1..256")
@click.option("--out", "out_dir", required=True, type=click.Path(path_type=Path), help="Directory the adapter is written to")
@click.option("--storage-dir", type=click.Path(path_type=Path), default=Path("storage"), help="Where MODEL and BASE live")
@click.option("--modules", type=str, default=None, help="Only the modules whose name ends in one of these, comma-separated (q_proj,k_proj,...)")
@click.option("--power-iters", type=int, default=2, help="Power iterations of the subspace iteration, 0..4")
@click.option("--dtype", "dtype_name", type=click.Choice(["bf16", "fp16", "fp32"]), default="bf16", help="The factors' dtype")
@click.option("--seed", type=int, default=0, help="Seed of the sketch")
@click.option("--device", type=str, default="cuda", help="Device to perform tensor operations on")
@click.option("--verbose", is_flag=True, help="Enable verbose logging")
def extract_lora_command(model: str, base: str, rank: int, out_dir: Path, storage_dir: Path, modules: Optional[str], power_iters: int,
                         dtype_name: str, seed: int, device: str, verbose: bool):
    """A PEFT LoRA adapter of rank RANK from the full finetune MODEL and its base: every Linear weight that differs.

    DIR receives adapter_model.safetensors, adapter_config.json and extraction.json (per tensor the singular values, the
    effective rank and the captured energy share); it can be named as a finetune_merge entry of `merge`.
    """
    setup_logging(verbose)
    from .constants import tune_hip_queues
    tune_hip_queues()                   # before the first GPU call, as merge does
    try:
        from .merge.extract import DTYPES, format_table, parse_modules, run_extraction
        result = asyncio.run(run_extraction(model, base, rank, out_dir, storage_dir, parse_modules(modules), power_iters,
                                            DTYPES[dtype_name], seed, device))
    except Exception as exc:
        logging.error(f"Error during extract-lora: {exc}", exc_info=verbose)
        traceback.print_exc()
        raise click.Abort()
    click.echo(format_table(result))
    click.echo(f"adapter: {out_dir}")


@cli.command("compress-delta")
@click.argument("model", type=str)
@click.option("--base", required=True, type=str, help="The base model MODEL was finetuned from (under the storage directory)")
@click.option("--out", "out_dir", required=True, type=click.Path(path_type=Path), help="Directory the delta pack is written to")
@click.option("--storage-dir", type=click.Path(path_type=Path), default=Path("storage"), help="Where MODEL and BASE live")
@click.option("--bits", type=int, default=1, help="1: the sign of every delta; 2: a mask of the largest deltas and their signs")
@click.option("--density", type=float, default=None, help="--bits 2: the share of the largest deltas to keep, in (0, 1]")
@click.option("--scale", type=click.Choice(["row", "tensor"]), default="row", help="One scale per row of shape[0], or per tensor")
@click.option("--modules", type=str, default=None, help="Pack only the modules whose name ends in one of these, comma-separated; the others are stored whole")
@click.option("--device", type=str, default="cuda", help="Device to perform tensor operations on")
@click.option("--verbose", is_flag=True, help="Enable verbose logging")
def compress_delta_command(model: str, base: str, out_dir: Path, storage_dir: Path, bits: int, density: Optional[float], scale: str,
                           modules: Optional[str], device: str, verbose: bool):
    """A delta pack of the full finetune MODEL on its base: one or two bits per weight and a scale per row.

    DIR receives delta_model.safetensors, delta_config.json and compression.json (per tensor what was kept, the threshold
    and the relative residual); it can be named as a finetune_merge entry of `merge` in place of MODEL.
    """
    setup_logging(verbose)
    from .constants import tune_hip_queues
    tune_hip_queues()                   # before the first GPU call, as merge does
    try:
        from .merge.compress import format_table, run_compression
        from .merge.extract import parse_modules
        result = asyncio.run(run_compression(model, base, out_dir, storage_dir, bits, density, scale, parse_modules(modules), device))
    except Exception as exc:
        logging.error(f"Error during compress-delta: {exc}", exc_info=verbose)
        traceback.print_exc()
        raise click.Abort()
    click.echo(format_table(result))
    click.echo(f"delta pack: {out_dir}")


@cli.command("emr-task")
@click.argument("model", type=str)
@click.option("--base", required=True, type=str, help="The base model MODEL was finetuned from (under the storage directory)")
@click.option("--unified", required=True, type=str, help="The unified model of an `operator: emr` merge (under the storage directory)")
@click.option("--out", "out_dir", required=True, type=click.Path(path_type=Path), help="Directory the EMR pack is written to")
@click.option("--storage-dir", type=click.Path(path_type=Path), default=Path("storage"), help="Where MODEL, BASE and the unified model live")
@click.option("--scale", type=click.Choice(["model", "tensor"]), default="model", help="One rescaler for the whole model, or one per tensor")
@click.option("--full", "full", type=str, default=None, help="Store whole the tensors whose name ends in one of these, comma-separated")
@click.option("--device", type=str, default="cuda", help="Device to perform tensor operations on")
@click.option("--verbose", is_flag=True, help="Enable verbose logging")
def emr_task_command(model: str, base: str, unified: str, out_dir: Path, storage_dir: Path, scale: str, full: Optional[str],
                     device: str, verbose: bool):
    """The modulator of task MODEL on an EMR-Merging merge: per tensor a 1-bit mask and one rescaler.

    DIR receives emr_model.safetensors, emr_config.json and emr_task.json (per tensor the mask's count, the rescaler and
    the relative residual); it can be named as a finetune_merge entry of `merge` in place of MODEL.
    """
    setup_logging(verbose)
    from .constants import tune_hip_queues
    tune_hip_queues()                   # before the first GPU call, as merge does
    try:
        from .merge.emr_task import format_table, parse_suffixes, run_emr_task
        result = asyncio.run(run_emr_task(model, base, unified, out_dir, storage_dir, scale, parse_suffixes(full), device))
    except Exception as exc:
        logging.error(f"Error during emr-task: {exc}", exc_info=verbose)
        traceback.print_exc()
        raise click.Abort()
    click.echo(format_table(result))
    click.echo(f"EMR pack: {out_dir}")


if __name__ == "__main__":
    cli()

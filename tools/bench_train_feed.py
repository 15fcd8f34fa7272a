"""Feeding the training step: what a batch of 16 x (4 + 1) planes at 256^2 costs the host way and the device way, and what the fed graph costs
against the fixed-input one.  Two steps, each its own process (run each under its own time limit; chain them with && from a script):

    python tools/bench_train_feed.py feed  [--repeats 5]   # (a) host arm against device arm, ms per batch; (b) the launch alone, device events
    python tools/bench_train_feed.py step  [--repeats 3]   # TrainingGraph.replay() against capture_step's replay on fixed inputs, full-width bf16
    python tools/bench_train_feed.py feed --augment        # afcm_batch_assemble_aug (identity and random rows) beside the plain launch; the host arm
    python tools/bench_train_feed.py feed --intensity      # afcm_batch_assemble_noise (identity rows, each transform, all three, the reference's
                                                           # probabilities) beside the plain and the augmented launch; the host arm
    python tools/bench_train_feed.py feed --elastic        # afcm_batch_assemble_elastic (no item, every item, the reference's probability 0.1;
                                                           # orders 3, 1, 0) beside the plain launch; the host arm
    python tools/bench_train_feed.py feed --blur           # afcm_batch_assemble_blur (no plane, every plane at radius 8, the reference's
                                                           # probability 0.5, the same with the elastic table) beside the plain and the elastic
                                                           # launch; the host arm.  --only ARM: that arm's launches alone, for a kernel trace
    python tools/bench_train_feed.py feed --normalise percentile|standardize
                                                           # afcm_plane_norm_stats alone, the normalised batch (statistics +
                                                           # afcm_batch_assemble_norm) beside the plain launch; the host arm

(a) alternates ``DeviceSliceSet.host_batch`` (SliceDataset items in numpy, stacked, uploaded) and ``DeviceSliceSet.batch`` (one launch) over the same
rows of a synthetic uint8 set after a warm-up of each, the alternation repeated; wall time by a host clock ended by a synchronise.  (b) times
``afcm_batch_assemble`` on 16 x (4 + 1) x 256^2, fp32 and bf16, and ``afcm_slice_assemble`` on 16 x 4 x 256^2 fp32, per output byte, in the loaded
library (``AFCM_HIP_LIB`` names another build to set beside it).  No timing here is gated by a test; the numbers go to DESIGN section 8i with their
spread."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_set(subjects, depth, res, device, **kw):
    import torch
    from afcm_amd import synthetic
    from afcm_amd.training import DeviceSliceSet
    to_u8 = lambda t: ((t + 1) * 127.5).round().clamp(0, 255).to(torch.uint8).numpy()
    sources = [{'t1': to_u8(synthetic.mr_like_slices(depth, 1, res, seed=2 * s)[:, 0]), 't2': to_u8(synthetic.mr_like_slices(depth, 1, res, seed=2 * s + 1)[:, 0])}
               for s in range(subjects)]
    return DeviceSliceSet(sources, patch_shape=(1, res, res), raw_internal_path_in=['t1'], raw_internal_path_out=['t2'], thickness=[2, 3, 5], device=device, **kw)


def spread(v):
    return max(v) - min(v)


def events_us(fn, launches=200):
    import torch
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def feed(args):
    import torch
    from afcm_amd import _lib
    from afcm_amd.torch_utils.ops.volume_ops import assemble_slices
    if not torch.cuda.is_available():
        raise SystemExit('bench_train_feed.py needs a GPU: a time taken without one says nothing')
    dev = torch.device('cuda:0')
    ds = synthetic_set(args.subjects, args.depth, args.res, dev)
    items = ds.epoch_items(0)
    ds.load_epoch(items)
    batches = min(args.batches, len(items) // args.batch)

    def clock(arm):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for j in range(batches):
            out = ds.batch(j * args.batch, args.batch) if arm == 'device' else ds.host_batch(items, j * args.batch, args.batch)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / batches, out

    arms, last = {'host': [], 'device': []}, {}
    for name in arms:
        clock(name)
    for _ in range(args.repeats):
        for name in arms:
            ms, last[name] = clock(name)
            arms[name].append(ms)
    equal = all(torch.equal(a, b) for a, b in zip(last['host'], last['device']))
    print(f'training batches of {args.batch} x (4 + 1) planes at {args.res}^2 from {args.subjects} uint8 subjects of ({args.depth}, {args.res}, {args.res}), '
          f'{batches} batches per pass, {args.repeats} repeats of the alternation after one warm-up pass of each arm')
    stats = {}
    for name, v in arms.items():
        stats[name] = dict(per_repeat_ms=v, mean_ms=sum(v) / len(v), spread_ms=spread(v))
        print(f'{name:8s} ms/batch per repeat {"  ".join(f"{x:8.4f}" for x in v)}   mean {stats[name]["mean_ms"]:8.4f}   spread {stats[name]["spread_ms"]:.4f}')
    print(f'the two arms\' last batches are {"bit-identical" if equal else "DIFFERENT"}')

    # the launch alone: the C entry point on the loaded epoch's tables, outputs reused
    launches, lib = {}, _lib.load()
    for out_name, out_dtype in (('fp32', torch.float32), ('bf16', torch.bfloat16)):
        a = torch.empty((args.batch, 4, args.res, args.res), dtype=out_dtype, device=dev)
        b = torch.empty((args.batch, 1, args.res, args.res), dtype=out_dtype, device=dev)
        c = torch.empty((args.batch, 1), dtype=torch.float32, device=dev)
        out_bytes = a.numel() * a.element_size() + b.numel() * b.element_size()
        stream = _lib.stream_ptr(a)

        def launch():
            rc = lib.afcm_batch_assemble(a.data_ptr(), b.data_ptr(), c.data_ptr(), ds.pool.data_ptr(), ds.pool.numel(), _lib.SRC_U8, ds.vols.data_ptr(),
                                         int(ds.vols.shape[0]), ds.items.data_ptr(), int(ds.items.shape[0]), None, 0, args.batch, 4, args.res, args.res,
                                         _lib.dtype_code(a), 0., 255., stream)
            assert rc == 0, rc
        us = [events_us(launch) for _ in range(args.repeats)]
        launches[f'batch_assemble_{out_name}'] = dict(per_repeat_us=us, mean_us=sum(us) / len(us), spread_us=spread(us),
                                                      ns_per_kib=sum(us) / len(us) * 1e3 / (out_bytes / 1024))
    volume = ds.pool[:args.depth * args.res * args.res].view(args.depth, args.res, args.res)
    us = [events_us(lambda: assemble_slices(volume, 0, args.batch, (1, args.res, args.res), thickness=5)) for _ in range(args.repeats)]
    launches['slice_assemble_fp32'] = dict(per_repeat_us=us, mean_us=sum(us) / len(us), spread_us=spread(us),
                                           ns_per_kib=sum(us) / len(us) * 1e3 / (args.batch * 4 * args.res * args.res * 4 / 1024))
    for name, s in launches.items():
        print(f'{name:22s} us per launch {"  ".join(f"{x:7.2f}" for x in s["per_repeat_us"])}   mean {s["mean_us"]:7.2f}   spread {s["spread_us"]:.2f}   '
              f'{s["ns_per_kib"]:.3f} ns per KiB of output')
    print(json.dumps(dict(bench='train_feed', res=args.res, batch=args.batch, arms=stats, launches=launches, equal=equal)))
    return 0 if equal else 1


def feed_augment(args):
    """``feed --augment``: the augmented launch (identity rows: the contiguous path; full random rows: the gather) beside the plain launch, device
    events, the arms alternated inside every repeat; and the host arm -- stacked ``SliceDataset`` items + ``augment.apply_host`` -- by a host clock."""
    import torch
    from afcm_amd import _lib
    import numpy as np
    from afcm_amd.augment import AugmentConfig, identity_rows, make_rows
    if not torch.cuda.is_available():
        raise SystemExit('bench_train_feed.py needs a GPU: a time taken without one says nothing')
    dev = torch.device('cuda:0')
    ds = synthetic_set(args.subjects, args.depth, args.res, dev, augment=AugmentConfig(flip_axes=(1, 2), rotate90=True, angle_spectrum=45))
    items, random_rows = ds.epoch_items(0), ds.epoch_augment(1)
    # flip_w alone: the gather's whole coordinate arithmetic on rows that are read contiguously (backwards) -- what separates the arithmetic from the
    # scattered reads of a rotation
    tables = {'identity': torch.from_numpy(identity_rows(len(items))).to(dev), 'flip_w': torch.from_numpy(make_rows(0, 1, 0, np.zeros(len(items)), (args.res, args.res))).to(dev),
              'random': torch.from_numpy(random_rows).to(dev)}
    ds.load_epoch(items, random_rows)
    batches = min(args.batches, len(items) // args.batch)
    lib, launches = _lib.load(), {}
    for out_name, out_dtype in (('fp32', torch.float32), ('bf16', torch.bfloat16)):
        a = torch.empty((args.batch, 4, args.res, args.res), dtype=out_dtype, device=dev)
        b = torch.empty((args.batch, 1, args.res, args.res), dtype=out_dtype, device=dev)
        c = torch.empty((args.batch, 1), dtype=torch.float32, device=dev)
        out_bytes = a.numel() * a.element_size() + b.numel() * b.element_size()
        head = (a.data_ptr(), b.data_ptr(), c.data_ptr(), ds.pool.data_ptr(), ds.pool.numel(), _lib.SRC_U8, ds.vols.data_ptr(), int(ds.vols.shape[0]),
                ds.items.data_ptr(), int(ds.items.shape[0]))
        tail = (None, 0, args.batch, 4, args.res, args.res, _lib.dtype_code(a), 0., 255., _lib.stream_ptr(a))

        def plain():
            assert lib.afcm_batch_assemble(*head, *tail) == 0

        def augmented(table):
            def launch():
                assert lib.afcm_batch_assemble_aug(*head, table.data_ptr(), *tail) == 0
            return launch

        arms = {'plain': plain, 'aug_identity': augmented(tables['identity']), 'aug_flip_w': augmented(tables['flip_w']),
                'aug_random': augmented(tables['random'])}
        us = {name: [] for name in arms}
        for _ in range(args.repeats):
            for name, fn in arms.items():
                us[name].append(events_us(fn))
        for name, v in us.items():
            launches[f'{name}_{out_name}'] = dict(per_repeat_us=v, mean_us=sum(v) / len(v), spread_us=spread(v),
                                                  ns_per_kib=sum(v) / len(v) * 1e3 / (out_bytes / 1024))

    def clock(rows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for j in range(batches):
            out = ds.host_batch(items, j * args.batch, args.batch, augment=rows)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / batches, out

    host = {'host_plain': None, 'host_random': random_rows}
    stats, last = {name: [] for name in host}, {}
    for name, rows in host.items():
        clock(rows)
    for _ in range(args.repeats):
        for name, rows in host.items():
            ms, last[name] = clock(rows)
            stats[name].append(ms)
    device_last = ds.batch((batches - 1) * args.batch, args.batch)
    equal = all(torch.equal(x, y) for x, y in zip(last['host_random'], device_last))
    print(f'augmented training batches of {args.batch} x (4 + 1) planes at {args.res}^2 from {args.subjects} uint8 subjects of ({args.depth}, {args.res}, '
          f'{args.res}); flips, quarter turns and angles in -45 ... 44 drawn per item; {args.repeats} repeats, the arms alternated inside each')
    for name, s in launches.items():
        print(f'{name:20s} us per launch {"  ".join(f"{x:7.2f}" for x in s["per_repeat_us"])}   mean {s["mean_us"]:7.2f}   spread {s["spread_us"]:.2f}   '
              f'{s["ns_per_kib"]:.3f} ns per KiB of output')
    arms = {}
    for name, v in stats.items():
        arms[name] = dict(per_repeat_ms=v, mean_ms=sum(v) / len(v), spread_ms=spread(v))
        print(f'{name:20s} ms/batch per repeat {"  ".join(f"{x:8.3f}" for x in v)}   mean {arms[name]["mean_ms"]:8.3f}   spread {arms[name]["spread_ms"]:.3f}')
    print(f'the host arm\'s and the device\'s last augmented batch are {"bit-identical" if equal else "DIFFERENT"}')
    print(json.dumps(dict(bench='train_feed_augment', res=args.res, batch=args.batch, launches=launches, arms=arms, equal=equal)))
    return 0 if equal else 1


def feed_intensity(args):
    """``feed --intensity``: the noise launch beside the plain and the augmented one, device events, the arms alternated inside every repeat --
    identity rows (the row check alone; once more with 23 cut points to check), every item executing one transform (contrast: the float64 round trip; Gaussian: one Philox call per four
    pixels, two logarithms, two sine / cosine pairs and two square roots; Poisson at lam 1 and 4: one call and 13 / 23 cut points), every item
    executing all three, and the reference's execution probabilities (0.2 each); and the host arm by a host clock."""
    import torch
    from afcm_amd import _lib
    import numpy as np
    from afcm_amd.augment import AugmentConfig
    from afcm_amd.augment_intensity import IntensityConfig, identity_rows, make_rows
    if not torch.cuda.is_available():
        raise SystemExit('bench_train_feed.py needs a GPU: a time taken without one says nothing')
    dev = torch.device('cuda:0')
    reference = IntensityConfig(contrast=(0.5, 1.5, 0.0, 0.2), gaussian=(0.0, 1.0, 0.2), poisson=(0.0, 1.0, 0.2))
    ds = synthetic_set(args.subjects, args.depth, args.res, dev, augment=AugmentConfig(flip_axes=(1, 2), rotate90=True, angle_spectrum=45), intensity=reference)
    items, geo_rows, reference_rows = ds.epoch_items(0), ds.epoch_augment(1), ds.epoch_intensity(2)
    n = len(items)
    keys = np.random.default_rng(3).integers(0, 2 ** 32, (n, 2))
    std, lam = np.random.default_rng(4).uniform(0.0, 1.0, n), np.random.default_rng(5).uniform(0.0, 1.0, n)
    all_rows = make_rows(contrast=(1, 1.25, 0.0), gaussian=(1, std), poisson=(1, lam), keys=keys, n=n)
    tables = {'noise_identity': identity_rows(n), 'noise_contrast': make_rows(contrast=(1, 1.25, 0.0), keys=keys, n=n),
              'noise_gaussian': make_rows(gaussian=(1, std), keys=keys, n=n), 'noise_poisson_lam1': make_rows(poisson=(1, 1.0), keys=keys, n=n),
              'noise_poisson_lam4': make_rows(poisson=(1, 4.0), keys=keys, n=n), 'noise_all_three': all_rows, 'noise_reference_0.2': reference_rows}
    # no flag set, but the 23 cut points of lam 4 in the row: the row check's reads and comparisons alone, without a Philox call or a search
    checked = make_rows(poisson=(1, 4.0), keys=keys, n=n)
    checked[:, 5] = 0.0
    tables['noise_identity_23_cuts'] = checked
    tables = {name: torch.from_numpy(rows).to(dev) for name, rows in tables.items()}
    geo = torch.from_numpy(geo_rows).to(dev)
    ds.load_epoch(items, None, all_rows)
    batches = min(args.batches, n // args.batch)
    lib, launches = _lib.load(), {}
    for out_name, out_dtype in (('fp32', torch.float32), ('bf16', torch.bfloat16)):
        a = torch.empty((args.batch, 4, args.res, args.res), dtype=out_dtype, device=dev)
        b = torch.empty((args.batch, 1, args.res, args.res), dtype=out_dtype, device=dev)
        c = torch.empty((args.batch, 1), dtype=torch.float32, device=dev)
        out_bytes = a.numel() * a.element_size() + b.numel() * b.element_size()
        head = (a.data_ptr(), b.data_ptr(), c.data_ptr(), ds.pool.data_ptr(), ds.pool.numel(), _lib.SRC_U8, ds.vols.data_ptr(), int(ds.vols.shape[0]),
                ds.items.data_ptr(), int(ds.items.shape[0]))
        tail = (None, 0, args.batch, 4, args.res, args.res, _lib.dtype_code(a), 0., 255., _lib.stream_ptr(a))

        def plain():
            assert lib.afcm_batch_assemble(*head, *tail) == 0

        def augmented():
            assert lib.afcm_batch_assemble_aug(*head, geo.data_ptr(), *tail) == 0

        def noisy(table, augment=None):
            def launch():
                assert lib.afcm_batch_assemble_noise(*head, augment, table.data_ptr(), 0, *tail) == 0
            return launch

        arms = dict({'plain': plain, 'aug_random': augmented}, **{name: noisy(table) for name, table in tables.items()})
        arms['aug_random+noise_all_three'] = noisy(tables['noise_all_three'], geo.data_ptr())
        us = {name: [] for name in arms}
        for _ in range(args.repeats):
            for name, fn in arms.items():
                us[name].append(events_us(fn))
        for name, v in us.items():
            launches[f'{name}_{out_name}'] = dict(per_repeat_us=v, mean_us=sum(v) / len(v), spread_us=spread(v),
                                                  ns_per_kib=sum(v) / len(v) * 1e3 / (out_bytes / 1024))

    def clock(rows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for j in range(batches):
            out = ds.host_batch(items, j * args.batch, args.batch, intensity=rows)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / batches, out

    host = {'host_plain': None, 'host_all_three': all_rows}
    stats, last = {name: [] for name in host}, {}
    for name, rows in host.items():
        clock(rows)
    for _ in range(args.repeats):
        for name, rows in host.items():
            ms, last[name] = clock(rows)
            stats[name].append(ms)
    device_last = ds.batch((batches - 1) * args.batch, args.batch)
    equal = all(torch.equal(x, y) for x, y in zip(last['host_all_three'], device_last))
    print(f'training batches of {args.batch} x (4 + 1) planes at {args.res}^2 from {args.subjects} uint8 subjects of ({args.depth}, {args.res}, {args.res}) with '
          f'intensity augmentation; std and lam in [0, 1) per item unless named; {args.repeats} repeats, the arms alternated inside each')
    for name, s in launches.items():
        print(f'{name:34s} us per launch {"  ".join(f"{x:7.2f}" for x in s["per_repeat_us"])}   mean {s["mean_us"]:7.2f}   spread {s["spread_us"]:.2f}   '
              f'{s["ns_per_kib"]:.3f} ns per KiB of output')
    arms = {}
    for name, v in stats.items():
        arms[name] = dict(per_repeat_ms=v, mean_ms=sum(v) / len(v), spread_ms=spread(v))
        print(f'{name:34s} ms/batch per repeat {"  ".join(f"{x:8.3f}" for x in v)}   mean {arms[name]["mean_ms"]:8.3f}   spread {arms[name]["spread_ms"]:.3f}')
    print(f'the host arm\'s and the device\'s last noisy batch are {"bit-identical" if equal else "DIFFERENT"}')
    print(json.dumps(dict(bench='train_feed_intensity', res=args.res, batch=args.batch, launches=launches, arms=arms, equal=equal)))
    return 0 if equal else 1


def feed_elastic(args):
    """``feed --elastic``: the elastic launches (``afcm_batch_assemble_elastic``: 8 at order 3) beside the plain launch, device events over the
    whole call, the arms alternated inside every repeat -- no item executing (the fixed cost: the scratch round trip and seven launches that exit
    early), every item executing (orders 3, 1 and 0) and the reference's execution probability 0.1, with the reference's sigma 50 and alpha 2000;
    and the host arm -- ``augment_elastic.apply_host`` -- by a host clock."""
    import torch
    from afcm_amd import _lib
    import numpy as np
    from afcm_amd.augment_elastic import ElasticConfig, elastic_rows, identity_rows
    from afcm_amd.torch_utils.ops.batch_ops import elastic_workspace_bytes
    if not torch.cuda.is_available():
        raise SystemExit('bench_train_feed.py needs a GPU: a time taken without one says nothing')
    dev = torch.device('cuda:0')
    ds = synthetic_set(args.subjects, args.depth, args.res, dev, elastic=ElasticConfig())
    items = ds.epoch_items(0)
    n = len(items)
    every = elastic_rows(ElasticConfig(execution_probability=1.0), n, np.random.default_rng(1))
    tables = {'elastic_none': identity_rows(n), 'elastic_every': every, 'elastic_reference_0.1': ds.epoch_elastic(2)}
    tables = {name: torch.from_numpy(rows).to(dev) for name, rows in tables.items()}
    ds.load_epoch(items, None, None, every)
    batches = min(args.batches, n // args.batch)
    lib, launches = _lib.load(), {}
    op_h, op_w, _ = ds.elastic_ops
    work = torch.empty(elastic_workspace_bytes(args.batch, 4, args.res, args.res, 3), dtype=torch.uint8, device=dev)
    for out_name, out_dtype in (('fp32', torch.float32), ('bf16', torch.bfloat16)):
        a = torch.empty((args.batch, 4, args.res, args.res), dtype=out_dtype, device=dev)
        b = torch.empty((args.batch, 1, args.res, args.res), dtype=out_dtype, device=dev)
        c = torch.empty((args.batch, 1), dtype=torch.float32, device=dev)
        out_bytes = a.numel() * a.element_size() + b.numel() * b.element_size()
        head = (a.data_ptr(), b.data_ptr(), c.data_ptr(), ds.pool.data_ptr(), ds.pool.numel(), _lib.SRC_U8, ds.vols.data_ptr(), int(ds.vols.shape[0]),
                ds.items.data_ptr(), int(ds.items.shape[0]))
        tail = (None, 0, args.batch, 4, args.res, args.res, _lib.dtype_code(a), 0., 255., _lib.stream_ptr(a))

        def plain():
            assert lib.afcm_batch_assemble(*head, *tail) == 0

        def elastic(table, order):
            def launch():
                assert lib.afcm_batch_assemble_elastic(*head, None, None, 0, table.data_ptr(), op_h.data_ptr(), op_w.data_ptr(), order, work.data_ptr(),
                                                       work.numel(), *tail) == 0
            return launch

        arms = dict({'plain': plain}, **{name: elastic(table, 3) for name, table in tables.items()})
        arms['elastic_every_order1'], arms['elastic_every_order0'] = elastic(tables['elastic_every'], 1), elastic(tables['elastic_every'], 0)
        us = {name: [] for name in arms}
        for _ in range(args.repeats):
            for name, fn in arms.items():
                us[name].append(events_us(fn, launches=50))
        for name, v in us.items():
            launches[f'{name}_{out_name}'] = dict(per_repeat_us=v, mean_us=sum(v) / len(v), spread_us=spread(v),
                                                  ns_per_kib=sum(v) / len(v) * 1e3 / (out_bytes / 1024))

    def clock(rows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for j in range(batches):
            out = ds.host_batch(items, j * args.batch, args.batch, elastic=rows)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / batches, out

    host = {'host_plain': None, 'host_every': every}
    stats, last = {name: [] for name in host}, {}
    for name, rows in host.items():
        clock(rows)
    for _ in range(args.repeats):
        for name, rows in host.items():
            ms, last[name] = clock(rows)
            stats[name].append(ms)
    device_last = ds.batch((batches - 1) * args.batch, args.batch)
    equal = all(torch.equal(x, y) for x, y in zip(last['host_every'], device_last))
    print(f'training batches of {args.batch} x (4 + 1) planes at {args.res}^2 from {args.subjects} uint8 subjects of ({args.depth}, {args.res}, {args.res}) with '
          f'the elastic deformation, sigma 50, alpha 2000, order 3 unless named; {args.repeats} repeats, the arms alternated inside each')
    for name, s in launches.items():
        print(f'{name:30s} us per call {"  ".join(f"{x:8.2f}" for x in s["per_repeat_us"])}   mean {s["mean_us"]:8.2f}   spread {s["spread_us"]:.2f}   '
              f'{s["ns_per_kib"]:.3f} ns per KiB of output')
    arms = {}
    for name, v in stats.items():
        arms[name] = dict(per_repeat_ms=v, mean_ms=sum(v) / len(v), spread_ms=spread(v))
        print(f'{name:30s} ms/batch per repeat {"  ".join(f"{x:8.3f}" for x in v)}   mean {arms[name]["mean_ms"]:8.3f}   spread {arms[name]["spread_ms"]:.3f}')
    print(f'the host arm\'s and the device\'s last deformed batch are {"bit-identical" if equal else "DIFFERENT"}')
    print(json.dumps(dict(bench='train_feed_elastic', res=args.res, batch=args.batch, launches=launches, arms=arms, equal=equal)))
    return 0 if equal else 1


def feed_blur(args):
    """``feed --blur``: the blur launches (``afcm_batch_assemble_blur``: 4, or 11 with an order-3 elastic table) beside the plain launch and the
    elastic launches, device events over the whole call, the arms alternated inside every repeat -- no plane executing (the cost every batch
    pays: the scratch round trip, the rows' check and a y pass that exits early), every plane executing at radius 8 (sigma 2, the upper end of the
    reference's range), the reference's execution probability 0.5 with sigma in [0.1, 2], and the same after the elastic deformation at its own
    reference settings; and the host arm -- ``augment_blur.apply_host`` -- by a host clock.  ``--only ARM`` launches that one arm 20 times and
    returns: what a kernel trace of one arm needs."""
    import torch
    from afcm_amd import _lib
    import numpy as np
    from afcm_amd.augment_blur import BlurConfig, identity_rows, plane_record
    from afcm_amd.augment_elastic import ElasticConfig
    from afcm_amd.torch_utils.ops.batch_ops import blur_workspace_bytes
    if not torch.cuda.is_available():
        raise SystemExit('bench_train_feed.py needs a GPU: a time taken without one says nothing')
    dev = torch.device('cuda:0')
    ds = synthetic_set(args.subjects, args.depth, args.res, dev, elastic=ElasticConfig(), blur=BlurConfig())
    items = ds.epoch_items(0)
    n = len(items)
    reference = ds.epoch_blur(1)
    tables = {'blur_none': identity_rows(n, 4), 'blur_every_radius8': np.tile(plane_record(2.0), (n, 5)), 'blur_reference_0.5': reference}
    tables = {name: torch.from_numpy(rows).to(dev) for name, rows in tables.items()}
    warp = torch.from_numpy(ds.epoch_elastic(2)).to(dev)
    ds.load_epoch(items, None, None, None, reference)
    batches = min(args.batches, n // args.batch)
    lib, launches = _lib.load(), {}
    op_h, op_w, order = ds.elastic_ops
    work = torch.empty(blur_workspace_bytes(args.batch, 4, args.res, args.res, order), dtype=torch.uint8, device=dev)
    for out_name, out_dtype in (('fp32', torch.float32), ('bf16', torch.bfloat16)):
        a = torch.empty((args.batch, 4, args.res, args.res), dtype=out_dtype, device=dev)
        b = torch.empty((args.batch, 1, args.res, args.res), dtype=out_dtype, device=dev)
        c = torch.empty((args.batch, 1), dtype=torch.float32, device=dev)
        out_bytes = a.numel() * a.element_size() + b.numel() * b.element_size()
        head = (a.data_ptr(), b.data_ptr(), c.data_ptr(), ds.pool.data_ptr(), ds.pool.numel(), _lib.SRC_U8, ds.vols.data_ptr(), int(ds.vols.shape[0]),
                ds.items.data_ptr(), int(ds.items.shape[0]))
        tail = (None, 0, args.batch, 4, args.res, args.res, _lib.dtype_code(a), 0., 255., _lib.stream_ptr(a))
        with_warp = (warp.data_ptr(), op_h.data_ptr(), op_w.data_ptr(), order)

        def plain():
            assert lib.afcm_batch_assemble(*head, *tail) == 0

        def elastic():
            assert lib.afcm_batch_assemble_elastic(*head, None, None, 0, *with_warp, work.data_ptr(), work.numel(), *tail) == 0

        def blur(table, warped=False):
            def launch():
                assert lib.afcm_batch_assemble_blur(*head, None, None, 0, *(with_warp if warped else (None, None, None, -1)), table.data_ptr(),
                                                    work.data_ptr(), work.numel(), *tail) == 0
            return launch

        arms = dict({'plain': plain, 'elastic_reference_0.1': elastic}, **{name: blur(table) for name, table in tables.items()})
        arms['blur_reference_0.5+elastic_0.1'] = blur(tables['blur_reference_0.5'], True)
        if args.only is not None:
            for _ in range(20):
                arms[args.only]()
            torch.cuda.synchronize()
            print(f'{args.only}: 20 calls, fp32 outputs')
            return 0
        us = {name: [] for name in arms}
        for _ in range(args.repeats):
            for name, fn in arms.items():
                us[name].append(events_us(fn, launches=50))
        for name, v in us.items():
            launches[f'{name}_{out_name}'] = dict(per_repeat_us=v, mean_us=sum(v) / len(v), spread_us=spread(v),
                                                  ns_per_kib=sum(v) / len(v) * 1e3 / (out_bytes / 1024))

    def clock(rows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for j in range(batches):
            out = ds.host_batch(items, j * args.batch, args.batch, blur=rows)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / batches, out

    host = {'host_plain': None, 'host_reference_0.5': reference}
    stats, last = {name: [] for name in host}, {}
    for name, rows in host.items():
        clock(rows)
    for _ in range(args.repeats):
        for name, rows in host.items():
            ms, last[name] = clock(rows)
            stats[name].append(ms)
    device_last = ds.batch((batches - 1) * args.batch, args.batch)
    equal = all(torch.equal(x, y) for x, y in zip(last['host_reference_0.5'], device_last))
    executed = float(reference[:, ::20].mean())
    print(f'training batches of {args.batch} x (4 + 1) planes at {args.res}^2 from {args.subjects} uint8 subjects of ({args.depth}, {args.res}, {args.res}) with '
          f'the per-plane Gaussian blur, sigma in [0.1, 2] ({100 * executed:.1f} % of the planes execute in the 0.5 table); elastic: sigma 50, alpha 2000, '
          f'order 3; {args.repeats} repeats, the arms alternated inside each')
    for name, s in launches.items():
        print(f'{name:36s} us per call {"  ".join(f"{x:8.2f}" for x in s["per_repeat_us"])}   mean {s["mean_us"]:8.2f}   spread {s["spread_us"]:.2f}   '
              f'{s["ns_per_kib"]:.3f} ns per KiB of output')
    arms = {}
    for name, v in stats.items():
        arms[name] = dict(per_repeat_ms=v, mean_ms=sum(v) / len(v), spread_ms=spread(v))
        print(f'{name:36s} ms/batch per repeat {"  ".join(f"{x:8.3f}" for x in v)}   mean {arms[name]["mean_ms"]:8.3f}   spread {arms[name]["spread_ms"]:.3f}')
    print(f'the host arm\'s and the device\'s last blurred batch are {"bit-identical" if equal else "DIFFERENT"}')
    print(json.dumps(dict(bench='train_feed_blur', res=args.res, batch=args.batch, launches=launches, arms=arms, equal=equal)))
    return 0 if equal else 1


def step(args):
    import torch
    from afcm_amd import layer_schedule as sched
    from afcm_amd.networks_stylegan3 import Stylegan3Generator
    from afcm_amd.stylegan3_model import StyleGAN3GeneratorStep, capture_step
    from afcm_amd.training import TrainingGraph
    if not torch.cuda.is_available():
        raise SystemExit('bench_train_feed.py needs a GPU: a time taken without one says nothing')
    dev = torch.device('cuda:0')
    ds = synthetic_set(args.subjects, args.depth, args.res, dev)
    items = ds.epoch_items(0)
    items = items[:len(items) // args.batch * args.batch]
    ds.load_epoch(items)

    def make_step():
        torch.manual_seed(0)
        G = Stylegan3Generator(z_dim=512, c_dim=1, w_dim=512, img_resolution=args.res, img_channels_in=4, img_channels_out=1, mapping_kwargs=dict(num_layers=8),
                               synthesis_kwargs=dict(dict(sched.DEFAULT_SYNTHESIS_KWARGS), compute_dtype=torch.bfloat16)).to(dev)
        return StyleGAN3GeneratorStep(G, capturable=True)

    a, b, c = ds.batch(0, args.batch)
    fixed = capture_step(make_step(), (a, b, torch.randn(args.batch, 512, device=dev), c), warmup=3)
    fed = TrainingGraph(make_step(), ds, args.batch, warmup=3)

    def replay_fed():
        if ds.position + args.batch > ds.rows:
            fed.rewind()
        fed.replay()

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    arms, fns = {'fixed': [], 'fed': []}, {'fixed': fixed.replay, 'fed': replay_fed}
    for name in arms:
        clock(fns[name])
    for _ in range(args.repeats):
        for name in arms:
            arms[name].append(clock(fns[name]))
    print(f'one generator step at {args.res}^2, batch {args.batch}, full-width bf16: capture_step replay on fixed inputs against TrainingGraph.replay() '
          f'(batch assembled inside the graph, gen_z redrawn outside it), {args.steps} steps per pass, {args.repeats} repeats of the alternation after a warm-up pass')
    stats = {}
    for name, v in arms.items():
        stats[name] = dict(per_repeat_ms=v, mean_ms=sum(v) / len(v), spread_ms=spread(v))
        print(f'{name:6s} ms/step per repeat {"  ".join(f"{x:8.3f}" for x in v)}   mean {stats[name]["mean_ms"]:8.3f}   spread {stats[name]["spread_ms"]:.3f}')
    diff, box = stats['fed']['mean_ms'] - stats['fixed']['mean_ms'], max(s['spread_ms'] for s in stats.values())
    print(f'fed - fixed = {diff:+.3f} ms/step ({100 * diff / stats["fixed"]["mean_ms"]:+.2f} %), largest spread of an arm {box:.3f} ms: '
          f'{"no difference" if abs(diff) <= box else "a difference"}')
    print(json.dumps(dict(bench='train_feed_step', res=args.res, batch=args.batch, arms=stats, fed_minus_fixed_ms=diff, largest_spread_ms=box)))
    return 0


def feed_normalise(args):
    """``feed --normalise percentile|standardize``: the statistics launch alone (``afcm_plane_norm_stats``, one workgroup per plane), the fed
    batch (statistics + ``afcm_batch_assemble_norm``) beside the plain launch, device events with the arms alternated inside every repeat; and
    the host arm -- stacked ``SliceDataset(normalise=)`` items -- by a host clock."""
    import torch
    from afcm_amd.normalise import NormaliseConfig
    from afcm_amd.torch_utils.ops.normalise_ops import norm_plan, plane_norm_stats
    if not torch.cuda.is_available():
        raise SystemExit('bench_train_feed.py needs a GPU: a time taken without one says nothing')
    dev = torch.device('cuda:0')
    config = NormaliseConfig(percentile=(1, 99.6)) if args.normalise == 'percentile' else NormaliseConfig(standardize=True)
    ds = synthetic_set(args.subjects, args.depth, args.res, dev, normalise=config)
    plain = synthetic_set(args.subjects, args.depth, args.res, dev)
    items = ds.epoch_items(0)
    ds.load_epoch(items)
    plain.load_epoch(items)
    hw = (args.res, args.res)
    coef = torch.empty((args.batch, 5, 4), dtype=torch.float64, device=dev)
    fns = {'stats_alone': lambda: plane_norm_stats(ds.pool, ds.vols, ds.items, 0, args.batch, hw, 4, config, out=coef),
           'plain_batch': lambda: plain.batch(0, args.batch),
           'normalised_batch': lambda: ds.batch(0, args.batch)}
    us = {name: [] for name in fns}
    for _ in range(args.repeats):
        for name, fn in fns.items():
            us[name].append(events_us(fn))
    print(f'{args.normalise}: batches of {args.batch} x (4 + 1) planes at {args.res}^2 from uint8 sources, {args.batch * 5} statistics workgroups, '
          f'plan {norm_plan(torch.uint8, config)}; 200 launches per figure, {args.repeats} repeats, the arms alternated')
    stats = {}
    for name, v in us.items():
        stats[name] = dict(per_repeat_us=v, mean_us=sum(v) / len(v), spread_us=spread(v))
        print(f'{name:18s} us per call {"  ".join(f"{x:8.2f}" for x in v)}   mean {stats[name]["mean_us"]:8.2f}   spread {stats[name]["spread_us"]:.2f}')
    want = ds.host_batch(items, 0, args.batch, normalise=config)
    t0 = time.perf_counter()
    for j in range(min(args.batches, 2)):
        ds.host_batch(items, j * args.batch, args.batch, normalise=config)
    torch.cuda.synchronize()
    host_ms = (time.perf_counter() - t0) * 1e3 / min(args.batches, 2)
    equal = all(torch.equal(a, b) for a, b in zip(ds.batch(0, args.batch), want))
    print(f'host arm {host_ms:.1f} ms per batch; the two arms\' batches are {"bit-identical" if equal else "DIFFERENT"}')
    print(json.dumps(dict(bench='train_feed_normalise', mode=args.normalise, res=args.res, batch=args.batch, launches=stats, host_ms=host_ms, equal=equal)))
    return 0 if equal else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['feed', 'step'])
    ap.add_argument('--subjects', type=int, default=4)
    ap.add_argument('--depth', type=int, default=64)
    ap.add_argument('--res', type=int, default=256)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--batches', type=int, default=8)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--augment', action='store_true', help='feed: time the augmented launch and the augmenting host arm instead')
    ap.add_argument('--intensity', action='store_true', help='feed: time the noise launch and its host arm instead')
    ap.add_argument('--elastic', action='store_true', help='feed: time the elastic launches and their host arm instead')
    ap.add_argument('--blur', action='store_true', help='feed: time the blur launches and their host arm instead')
    ap.add_argument('--only', default=None, help='feed --blur: launch this one arm 20 times and return (for a kernel trace)')
    ap.add_argument('--normalise', choices=['percentile', 'standardize'], default=None,
                    help='feed: time the per-plane statistics launch, the normalised batch and its host arm instead')
    args = ap.parse_args()
    if args.normalise is not None:
        if args.what != 'feed' or args.augment or args.intensity or args.elastic or args.blur:
            raise SystemExit('--normalise belongs to the feed step, on its own')
        return feed_normalise(args)
    if (args.augment or args.intensity or args.elastic or args.blur) and args.what != 'feed':
        raise SystemExit('--augment, --intensity, --elastic and --blur belong to the feed step')
    if args.augment + args.intensity + args.elastic + args.blur > 1:
        raise SystemExit('--augment, --intensity, --elastic or --blur, one at a time')
    if args.only is not None and not args.blur:
        raise SystemExit('--only belongs to feed --blur')
    feeds = feed_blur if args.blur else feed_elastic if args.elastic else (feed_intensity if args.intensity else (feed_augment if args.augment else feed))
    return {'feed': feeds, 'step': step}[args.what](args)


if __name__ == '__main__':
    sys.exit(main())

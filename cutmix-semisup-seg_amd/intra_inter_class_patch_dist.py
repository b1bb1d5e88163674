"""
Mirror of the reference's intra_inter_class_patch_dist.py: for anchor patches centred on class-boundary pixels, the nearest
same-class and other-class patches in the anchor's own image and over the rest of the training set -- the cluster-assumption
statistics of the paper. Same click options, same pickle (the eight `*_dists` / `*_coords` lists, coords (img_i, y, x) and dists
float64 in the units of img_as_float; `anchor_negative_img_dir_y_x_cls`; `boundary_dists`).

The training images sit decoded in an HBM-resident pool (resident_pool.ResidentPool) and every distance map is computed and
searched on the device, on exact integers (patch_dist.py here). Patches go through in chunks, images in the order of `train_ndx`;
the cross-image lists keep a running best `--n_neighbours` per patch ordered by (distance, visit order, flat pixel index), the
same-image lists are replaced, as in the reference.

Deviations from the reference:
  * only `--dataset pascal` and `pascal_aug` are built here and the default is `pascal_aug`, not `cityscapes`; any other choice
    stops with a refusal before the GPU is touched (the trainers do read camvid, cityscapes and isic2017)
  * `--patch_size` must be odd; an even one is refused the same way (the reference's even-size geometry is off by one)
  * `--show_progress` falls back to no bar when tqdm is not importable
  * equal distances are ordered by pixel index, not by an unstable argsort
"""
import click


@click.command(help='Intra-class / inter-class patch distances on the device. Deviations from the reference: only --dataset pascal '
                    'and pascal_aug are built (default pascal_aug; other choices are refused before the GPU is touched); --patch_size '
                    'must be odd; --show_progress needs tqdm and falls back to no bar without it.')
@click.argument('out_path', type=click.Path(writable=True))
@click.option('--dataset', type=click.Choice(['camvid', 'cityscapes', 'pascal', 'pascal_aug', 'gtav',
                                              'inria_aerial', 'isic2017']), default='pascal_aug')
@click.option('--patch_size', type=int, default=225)
@click.option('--n_patches', type=int, default=1000)
@click.option('--n_neighbours', type=int, default=1000)
@click.option('--batch_size', type=int, default=-1)
@click.option('--batch', type=int, default=0)
@click.option('--show_progress', is_flag=True, default=False)
@click.option('--batch_index_one_based', is_flag=True, default=False)
@click.option('--load_choice', type=click.Path(readable=True, exists=True))
@click.option('--save_choice', type=click.Path(writable=True))
@click.option('--seed', type=int, default=12345)
def intra_inter_class_patch_dist(out_path, dataset, patch_size, n_patches, n_neighbours,
                                 batch_size, batch, show_progress, batch_index_one_based,
                                 load_choice, save_choice, seed):
    import pickle
    import sys
    import numpy as np

    from . import job_helper, settings as settings_mod
    from .datapipe import datasets

    # refusals come first: nothing below them has touched the GPU
    if dataset not in datasets.TREE_SETS:
        raise SystemExit('The patch-distance analysis is built for {} only; `{}` is not (the trainers read it, this program does '
                         'not).'.format(' and '.join(datasets.TREE_SETS), dataset))
    if patch_size < 1 or patch_size % 2 == 0:
        raise SystemExit('--patch_size must be odd (got {}): the even-size patch geometry of the reference is off by one and is not '
                         'built.'.format(patch_size))
    if n_neighbours < 1:
        raise SystemExit('--n_neighbours must be positive')

    if batch_index_one_based:
        batch -= 1

    print('Command line:')
    print(' '.join(sys.argv))

    print('Loading dataset...', flush=True)
    try:
        ds = datasets.load_dataset(dataset, n_val=0, val_seed=0, n_sup=-1, n_unsup=-1, split_seed=12345, split_path=None)['ds_src']
    except (settings_mod.DataPathError, job_helper.JobNotRun) as e:
        raise SystemExit(str(e))

    progress_fn = lambda x, *args, **kwargs: x          # noqa: E731
    if show_progress:
        try:
            import tqdm
            progress_fn = tqdm.tqdm
        except ImportError:
            print('tqdm is not installed: no progress bar')

    import torch
    from . import patch_dist
    from .resident_pool import ResidentPool
    if not torch.cuda.is_available():
        raise SystemExit('intra_inter_class_patch_dist needs a GPU: the distance maps are computed on the device only')
    device = torch.device('cuda', torch.cuda.current_device())
    pool = ResidentPool(ds, ds.train_ndx, device, with_labels=True)
    patch_shape = (patch_size, patch_size)

    rng = np.random.RandomState(seed)
    if load_choice is not None:
        print('Loading choice of anchor and negative patches from {}'.format(load_choice))
        with open(load_choice, 'rb') as f_in:
            anchor_negative_ids = pickle.load(f_in)
    else:
        print('Choosing anchor and negative patches...', flush=True)
        anchor_negative_ids = patch_dist.choose_anchors_and_negatives(pool.labels, progress_fn(ds.train_ndx), n_patches, patch_shape,
                                                                      rng)
        if save_choice is not None:
            print('Saving choice of anchor and negative patches to {}'.format(save_choice))
            with open(save_choice, 'wb') as f_out:
                pickle.dump(anchor_negative_ids, f_out)

    # Select batch we are working on
    if batch_size == -1:
        batch_size = len(anchor_negative_ids)
    batch_ids = anchor_negative_ids[batch * batch_size:(batch + 1) * batch_size]
    if len(batch_ids) == 0:
        raise SystemExit('batch {} of size {} holds no patches ({} were chosen)'.format(batch, batch_size, len(anchor_negative_ids)))

    print('Extracting anchor and negative patches...', flush=True)
    patches = patch_dist.PatchSet(pool, batch_ids, patch_shape)

    print('Computing distances...', flush=True)
    results = class_distances(pool, ds.train_ndx, patches, n_neighbours, progress_fn)
    results['anchor_negative_img_dir_y_x_cls'] = batch_ids
    results['boundary_dists'] = patches.boundary_dists

    with open(out_path, 'wb') as f_out:
        pickle.dump(results, f_out)


def class_distances(pool, sample_indices, patches, n_neighbours, progress_fn=lambda x: x, chunk_size=None):
    """intra_inter_class_patch_dist.py:169-278 on the device -> the eight lists (one entry per patch)"""
    import numpy as np
    import torch
    from . import patch_dist as pd

    k = int(n_neighbours)
    dev = pool.device
    names = ('same_image_intra_class', 'same_image_inter_class', 'other_image_intra_class', 'other_image_inter_class')
    out = {name + suffix: [] for name in names for suffix in ('_dists', '_coords')}
    widths = {int(i): pool.sizes_of([i])[0][1] for i in sample_indices}
    anchor_img = torch.from_numpy(np.ascontiguousarray(patches.rows[:, 0], dtype=np.int64)).to(dev)

    for cache in progress_fn(pd.chunks_of(patches, chunk_size or pd.DEFAULT_CHUNK)):
        n = cache.last - cache.first
        own = anchor_img[cache.first:cache.last]
        empty = lambda: torch.full((n, k), pd.KEY_SENTINEL, dtype=torch.int64, device=dev)       # noqa: E731
        no_img = lambda: torch.full((n, k), -1, dtype=torch.int64, device=dev)                    # noqa: E731
        # [keys, image of each key] per list; the same-image lists are replaced, the other-image lists merged
        same = {'intra': [empty(), no_img()], 'inter': [empty(), no_img()]}
        other = {'intra': [empty(), no_img()], 'inter': [empty(), no_img()]}
        seen_own = torch.zeros((n,), dtype=torch.bool, device=dev)
        for img_i in sample_indices:
            img_i = int(img_i)
            nb = pd.class_neighbours(pool, img_i, patches, k, chunks=[cache])
            is_own = (own == img_i)[:, None]
            seen_own |= is_own[:, 0]
            for side, new_keys in (('intra', nb.intra_keys), ('inter', nb.inter_keys)):
                new_img = torch.full_like(new_keys, img_i)
                same[side][0] = torch.where(is_own, new_keys, same[side][0])
                same[side][1] = torch.where(is_own, new_img, same[side][1])
                merged_keys, merged_img = pd.merge_best(other[side][0], other[side][1], new_keys, img_i, k)
                other[side][0] = torch.where(is_own, other[side][0], merged_keys)
                other[side][1] = torch.where(is_own, other[side][1], merged_img)
        seen = seen_own.cpu().numpy()
        for where, lists in (('same_image', same), ('other_image', other)):
            for side in ('intra', 'inter'):
                keys, img = lists[side][0].cpu().numpy(), lists[side][1].cpu().numpy()
                for r in range(n):
                    name = '{}_{}_class'.format(where, side)
                    if where == 'same_image' and not seen[r]:
                        # the reference leaves None where the anchor's own image is not among those visited
                        out[name + '_dists'].append(None)
                        out[name + '_coords'].append(None)
                        continue
                    valid = keys[r] != pd.KEY_SENTINEL
                    kk, ii = keys[r][valid], img[r][valid]
                    d2 = kk >> pd.KEY_INDEX_BITS
                    flat = kk & ((1 << pd.KEY_INDEX_BITS) - 1)
                    w = np.array([widths[int(i)] for i in ii], dtype=np.int64)
                    out[name + '_dists'].append(np.sqrt(d2.astype(np.float64)) / 255.0)
                    out[name + '_coords'].append(np.stack([ii, flat // np.maximum(w, 1), flat % np.maximum(w, 1)], axis=1).astype(int)
                                                 if len(kk) else np.zeros((0, 3), dtype=int))
    return out


if __name__ == '__main__':
    intra_inter_class_patch_dist()

#!/usr/bin/env python
"""
Generate the data-only fixture of the data set path's tests:

    tests/golden/pascal_source.json
        tree      the fabricated Pascal VOC tree the tests rebuild themselves (name lists, image sizes)
        source    sample_names / train_ndx / val_ndx / test_ndx of the reference's own PascalVOCDataSource on that tree, for
                  augmented x n_val x trainval_perm
        streams   the first index batches of the reference's RepeatSampler(SubsetRandomSampler) in a DataLoader over an
                  index-returning data set, under torch.manual_seed: one loader, and two loaders sharing one sampler
        collate   canvas and offsets the reference's SegCollate gives batches of differently sized images

    python tests/golden/make_pascal_golden.py <path of a checkout of the reference>

Needs the reference's sources (its datapipe/pascal_voc_dataset.py and datapipe/seg_data.py import with PIL, tqdm and torch); the
output (names, sizes and recorded numbers only) is committed and is all the tests read.
"""
import json
import os
import sys
import tempfile

import numpy as np

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))

# name -> (H, W); deliberately not in sorted order in the lists below
SIZES = {
    '2007_000032': [70, 90], '2007_000039': [93, 71], '2007_000063': [75, 100], '2007_000068': [100, 75],
    '2007_000121': [81, 97], '2007_000170': [120, 100], '2007_000241': [77, 113], '2007_000243': [88, 88],
    '2007_000250': [99, 83], '2007_000256': [70, 120], '2007_000333': [111, 73], '2007_000363': [85, 95],
    '2008_000002': [90, 70], '2008_000003': [72, 91], '2008_000007': [101, 99], '2008_000008': [80, 80],
    '2008_000009': [119, 71], '2009_000001': [74, 106], '2009_000002': [96, 84],
}
TRAIN = ['2007_000363', '2007_000032', '2007_000250', '2007_000039', '2007_000333', '2007_000063', '2007_000256',
         '2007_000068', '2007_000243', '2007_000121', '2007_000241', '2007_000170']
VAL = ['2008_000008', '2008_000002', '2008_000009', '2008_000003', '2008_000007']
TRAIN_AUG = TRAIN[6:] + ['2009_000002'] + TRAIN[:6] + ['2009_000001']
PERM = {False: [7, 2, 11, 0, 5, 9, 3, 1, 10, 6, 4, 8], True: [13, 7, 2, 11, 0, 5, 9, 12, 3, 1, 10, 6, 4, 8]}
VAL_SEED = 131
STREAM_NDX = [3, 8, 11, 14, 20, 21, 30]
COLLATE_BATCHES = [[[70, 90], [93, 71], [75, 100]], [[100, 75], [81, 97]], [[64, 96], [33, 32], [1, 1]], [[77, 113]]]


def write_lists(root):
    for sub, train_file, train in (('Segmentation', 'train.txt', TRAIN), ('SegmentationAug', 'train_aug.txt', TRAIN_AUG)):
        d = os.path.join(root, 'ImageSets', sub)
        os.makedirs(d)
        with open(os.path.join(d, train_file), 'w') as f:
            f.write('\n'.join(train) + '\n\n')
        with open(os.path.join(d, 'val.txt'), 'w') as f:
            f.write('\n'.join(VAL) + '\n')


def main(ref):
    ref = os.path.abspath(ref)
    # keep the repository root (which holds same-named drop-in modules) OFF the path; the reference goes first
    sys.path = [p for p in sys.path if os.path.abspath(p or '.') not in (REPO, HERE)]
    sys.path.insert(0, ref)
    import torch
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, 'VOC2012')
        write_lists(root)
        with open(os.path.join(tmp, 'semantic_segmentation.cfg'), 'w') as f:
            f.write('[paths]\npascal_voc={}\n'.format(root))
        os.chdir(tmp)                                    # the reference reads ./semantic_segmentation.cfg
        from datapipe import pascal_voc_dataset, seg_data      # reference
        assert os.path.abspath(pascal_voc_dataset.__file__).startswith(ref)
        source = []
        for augmented in (False, True):
            for n_val in (0, 3):
                for with_perm in (False, True):
                    ds = pascal_voc_dataset.PascalVOCDataSource(
                        n_val=n_val, val_rng=np.random.RandomState(VAL_SEED),
                        trainval_perm=np.array(PERM[augmented]) if with_perm else None, augmented=augmented)
                    mean, std = ds.get_mean_std()
                    source.append(dict(augmented=augmented, n_val=n_val, with_perm=with_perm, sample_names=list(ds.sample_names),
                                       train_ndx=[int(v) for v in ds.train_ndx], val_ndx=[int(v) for v in ds.val_ndx],
                                       test_ndx=None if ds.test_ndx is None else [int(v) for v in ds.test_ndx],
                                       num_classes=int(ds.num_classes), mean=[float(v) for v in mean], std=[float(v) for v in std]))
        os.chdir(HERE)

    class IndexDataset(torch.utils.data.Dataset):
        def __len__(self):
            return 64

        def __getitem__(self, i):
            return int(i)

    def loader(sampler):
        return torch.utils.data.DataLoader(IndexDataset(), 3, sampler=sampler, num_workers=0)

    torch.manual_seed(1234)
    it = iter(loader(seg_data.RepeatSampler(torch.utils.data.SubsetRandomSampler(STREAM_NDX))))
    single = [[int(v) for v in next(it)] for _ in range(7)]           # 21 indices: crosses two permutation boundaries
    torch.manual_seed(4321)
    shared = seg_data.RepeatSampler(torch.utils.data.SubsetRandomSampler(STREAM_NDX))
    it_sup = iter(loader(seg_data.RepeatSampler(torch.utils.data.SubsetRandomSampler(STREAM_NDX[:4]))))
    it0, it1 = iter(loader(shared)), iter(loader(shared))
    trio = []
    for _ in range(6):                                                # the trainer's order: sup, unsup 0, unsup 1
        trio.append([[int(v) for v in next(i)] for i in (it_sup, it0, it1)])
    streams = dict(ndx=STREAM_NDX, batch_size=3, seed=1234, batches=single, trio_seed=4321, trio_sup_ndx=STREAM_NDX[:4], trio=trio)

    collate = []
    for block in ((1, 1), (32, 32)):
        for sizes in COLLATE_BATCHES:
            batch = [dict(image=np.ones((3, h, w), dtype=np.float32), labels=np.zeros((1, h, w), dtype=np.int32))
                     for h, w in sizes]
            out = seg_data.SegCollate(block)(batch)
            img, lab = out['image'].numpy(), out['labels'].numpy()
            offsets = []
            for k, (h, w) in enumerate(sizes):
                ys, xs = np.nonzero(img[k, 0])
                top, left = int(ys.min()), int(xs.min())
                assert (img[k, :, top:top + h, left:left + w] == 1).all() and img[k].sum() == 3 * h * w
                assert (lab[k, 0, top:top + h, left:left + w] == 0).all() and (lab[k] == 255).sum() == lab[k].size - h * w
                offsets.append([top, left])
            collate.append(dict(block_size=list(block), sizes=sizes, canvas=[int(img.shape[2]), int(img.shape[3])],
                                offsets=offsets))

    tree = dict(sizes=SIZES, train=TRAIN, val=VAL, train_aug=TRAIN_AUG, perm={'plain': PERM[False], 'aug': PERM[True]},
                val_seed=VAL_SEED)
    with open(os.path.join(HERE, 'pascal_source.json'), 'w') as f:
        json.dump(dict(tree=tree, source=source, streams=streams, collate=collate), f, indent=0)
    print('wrote pascal_source.json ({} source cases, {} collate cases)'.format(len(source), len(collate)))


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

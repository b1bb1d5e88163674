#!/usr/bin/env python
"""
Generate the data-only fixture of the ZIP data sources' tests:

    tests/golden/zip_sources.json
        perm, val_seed   what the cases were made with
        cases            for camvid / cityscapes / isic2017 x n_val in {0, 2} x with / without trainval_perm: sample_names,
                         train_ndx / val_ndx / test_ndx, num_classes, mean / std (and non_void_mapping for Cityscapes) of the
                         reference's own data sources on the archives tests/_zip_archives.py fabricates
        labels           the reference accessor's get_labels_arr of two samples per data set (for Cityscapes one stored as an
                         8-bit and one as a 16-bit PNG)

    python tests/golden/make_zip_sources_golden.py <path of a checkout of the reference>

Needs the reference's sources (its datapipe/{camvid,cityscapes,isic2017}_dataset.py and datapipe/seg_data.py import with PIL and
torch); the output (names and recorded numbers only) is committed and is all the tests read. The tests rebuild the same archives
with the same helper.
"""
import importlib.util
import json
import os
import sys
import tempfile

import numpy as np

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REPO = os.path.dirname(TESTS)


def load_helper():
    spec = importlib.util.spec_from_file_location('_zip_archives', os.path.join(TESTS, '_zip_archives.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(ref):
    ref = os.path.abspath(ref)
    Z = load_helper()
    # keep the repository root (which holds same-named drop-in modules) OFF the path; the reference goes first
    sys.path = [p for p in sys.path if os.path.abspath(p or '.') not in (REPO, HERE, TESTS)]
    sys.path.insert(0, ref)
    with tempfile.TemporaryDirectory() as tmp:
        Z.write_all(tmp)
        os.chdir(tmp)                                    # the reference reads ./semantic_segmentation.cfg
        from datapipe import camvid_dataset, cityscapes_dataset, isic2017_dataset      # reference
        assert os.path.abspath(cityscapes_dataset.__file__).startswith(ref)
        classes = dict(camvid=camvid_dataset.CamVidDataSource, cityscapes=cityscapes_dataset.CityscapesDataSource,
                       isic2017=isic2017_dataset.ISIC2017DataSource)
        cases, labels = [], {}
        for dataset in sorted(classes):
            for n_val in (0, 2):
                for with_perm in (False, True):
                    ds = classes[dataset](n_val=n_val, val_rng=np.random.RandomState(Z.VAL_SEED),
                                          trainval_perm=np.array(Z.PERM) if with_perm else None)
                    mean, std = ds.get_mean_std()
                    case = dict(dataset=dataset, n_val=n_val, with_perm=with_perm, sample_names=list(ds.sample_names),
                                train_ndx=[int(v) for v in ds.train_ndx], val_ndx=[int(v) for v in ds.val_ndx],
                                test_ndx=None if ds.test_ndx is None else [int(v) for v in ds.test_ndx],
                                num_classes=int(ds.num_classes), mean=[float(v) for v in mean], std=[float(v) for v in std])
                    if dataset == 'cityscapes':
                        case['non_void_mapping'] = [int(v) for v in ds.non_void_mapping]
                    cases.append(case)
            acc = ds.dataset(labels=True, mask=False, xf=False)
            wanted = {'cityscapes': [n for n, _ in Z.CITYSCAPES[:2]], 'isic2017': [n for n, _ in Z.ISIC2017[:2]],
                      'camvid': [n for _, n, _ in Z.CAMVID[:2]]}[dataset]
            labels[dataset] = []
            for name in wanted:
                i = ds.sample_names.index(name)
                y = np.asarray(acc.get_labels_arr(i))
                labels[dataset].append(dict(sample_name=name, index=int(i), shape=list(y.shape),
                                            values=[int(v) for v in y.reshape(-1)]))
        os.chdir(HERE)
    with open(os.path.join(HERE, 'zip_sources.json'), 'w') as f:
        json.dump(dict(perm=Z.PERM, val_seed=Z.VAL_SEED, cases=cases, labels=labels), f, separators=(',', ':'))
    print('wrote zip_sources.json ({} cases)'.format(len(cases)))


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

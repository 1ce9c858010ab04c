#!/usr/bin/env python3
"""Generate ``imageio.json`` FROM THE REFERENCE ITSELF (build container only: needs the reference's sources).

    python tests/golden/make_golden_imageio.py

Recorded: what the reference's own ``create_lists_from_splitted_dataset_folder`` (utilities/utils.py:42-56) and
``nnUNetPredictor._manage_input_and_output_lists`` (inference/predict_from_raw_data.py:166-205) return for the folders of
empty files, part splits and existing-output sets listed below.  Both import with the existing shims (the method only
reads ``self.dataset_json``, so it is called on a stand-in object).  Paths are stored relative to the scratch folder
(``<root>``), next to the arguments of every call and the files its output folder held.  Data only; no reference source travels.
"""
from __future__ import annotations

import json
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ref_shims  # noqa: E402

ref_shims.install()

from nnunetv2.inference.predict_from_raw_data import nnUNetPredictor  # noqa: E402
from nnunetv2.utilities.utils import create_lists_from_splitted_dataset_folder  # noqa: E402

# folder name -> the files in it (all empty)
FOLDERS = {
    'two_channels': ['case_a_0000.nii.gz', 'case_a_0001.nii.gz', 'case_b_0000.nii.gz', 'case_b_0001.nii.gz',
                     'liver_10_0000.nii.gz', 'liver_10_0001.nii.gz', 'liver_2_0000.nii.gz', 'liver_2_0001.nii.gz',
                     'liver_2_extra_0000.nii.gz', 'liver_2_extra_0001.nii.gz', 'notes.txt', 'case_a_0000.json'],
    'one_channel': ['s01_0000.nii.gz', 's02_0000.nii.gz', 's03_0000.nii.gz', 's04_0000.nii.gz', 's05_0000.nii.gz',
                    'S00_0000.nii.gz', 's1_0000.nii.gz'],
    'plain_nii': ['a.b_0000.nii', 'a.b_0001.nii', 'a+b_0000.nii', 'a+b_0001.nii', 'axb_0000.nii', 'c_0000.nii.gz'],
    # names that end in the file ending but not in _dddd<ending>: they still name an identifier, which then has no file
    'odd_names': ['case_c_000.nii.gz', 'case_d_0000.nii.gz', 'case_d_00001.nii.gz', 'case_e_000a.nii.gz'],
    'empty': [],
}
LIST_CASES = [('two_channels', '.nii.gz'), ('one_channel', '.nii.gz'), ('plain_nii', '.nii'), ('plain_nii', '.nii.gz'),
              ('odd_names', '.nii.gz'), ('empty', '.nii.gz')]

# existing-output sets (files made in the output folder before the call)
EXISTING = {
    'none': [],
    'labels_some': ['case_a.nii.gz', 'liver_2.nii.gz'],
    'labels_and_npz': ['case_a.nii.gz', 'case_a.npz', 'liver_2.nii.gz', 'liver_10.npz', 'case_b.nii.gz', 'case_b.npz',
                       'liver_2_extra.nii.gz'],
    'all': ['case_a.nii.gz', 'case_b.nii.gz', 'liver_10.nii.gz', 'liver_2.nii.gz', 'liver_2_extra.nii.gz'],
}
# source: 'folder' or 'list' (the lists the reference makes of the folder); output: 'folder', 'list' or None
MANAGE_CASES = [
    dict(src='two_channels', ending='.nii.gz', source='folder', output='folder', prev=False, overwrite=True, part_id=0, num_parts=1, save_probabilities=False, existing='none'),
    dict(src='two_channels', ending='.nii.gz', source='list', output='list', prev=True, overwrite=True, part_id=0, num_parts=1, save_probabilities=False, existing='none'),
    dict(src='two_channels', ending='.nii.gz', source='folder', output=None, prev=False, overwrite=False, part_id=0, num_parts=1, save_probabilities=True, existing='all'),
    dict(src='two_channels', ending='.nii.gz', source='folder', output='folder', prev=True, overwrite=True, part_id=0, num_parts=2, save_probabilities=False, existing='none'),
    dict(src='two_channels', ending='.nii.gz', source='folder', output='folder', prev=True, overwrite=True, part_id=1, num_parts=2, save_probabilities=False, existing='none'),
    dict(src='two_channels', ending='.nii.gz', source='list', output='list', prev=False, overwrite=True, part_id=2, num_parts=3, save_probabilities=False, existing='none'),
    dict(src='two_channels', ending='.nii.gz', source='folder', output='folder', prev=False, overwrite=True, part_id=4, num_parts=7, save_probabilities=False, existing='none'),
    dict(src='two_channels', ending='.nii.gz', source='folder', output='folder', prev=True, overwrite=False, part_id=0, num_parts=1, save_probabilities=False, existing='labels_some'),
    dict(src='two_channels', ending='.nii.gz', source='folder', output='folder', prev=False, overwrite=False, part_id=0, num_parts=1, save_probabilities=True, existing='labels_some'),
    dict(src='two_channels', ending='.nii.gz', source='folder', output='folder', prev=True, overwrite=False, part_id=0, num_parts=1, save_probabilities=False, existing='labels_and_npz'),
    dict(src='two_channels', ending='.nii.gz', source='list', output='list', prev=True, overwrite=False, part_id=0, num_parts=1, save_probabilities=True, existing='labels_and_npz'),
    dict(src='two_channels', ending='.nii.gz', source='folder', output='folder', prev=False, overwrite=False, part_id=1, num_parts=2, save_probabilities=True, existing='labels_and_npz'),
    dict(src='two_channels', ending='.nii.gz', source='folder', output='folder', prev=False, overwrite=False, part_id=0, num_parts=1, save_probabilities=False, existing='all'),
    dict(src='two_channels', ending='.nii.gz', source='folder', output='folder', prev=False, overwrite=True, part_id=0, num_parts=1, save_probabilities=True, existing='all'),
    dict(src='one_channel', ending='.nii.gz', source='folder', output='folder', prev=False, overwrite=True, part_id=1, num_parts=3, save_probabilities=False, existing='none'),
    dict(src='plain_nii', ending='.nii', source='folder', output='folder', prev=True, overwrite=True, part_id=0, num_parts=1, save_probabilities=False, existing='none'),
    dict(src='empty', ending='.nii.gz', source='folder', output='folder', prev=False, overwrite=True, part_id=0, num_parts=1, save_probabilities=False, existing='none'),
]


def make_folder(root, name, files):
    d = os.path.join(root, name)
    os.makedirs(d, exist_ok=True)
    for f in files:
        open(os.path.join(d, f), 'w').close()
    return d


def relative(obj, root):
    if isinstance(obj, str):
        return obj.replace(root, '<root>')
    if isinstance(obj, (list, tuple)):
        return [relative(i, root) for i in obj]
    return obj


def truncated_list(lists, ending, out_dir):
    """A caller's own list of truncated output names, one per case: 'pred_<case id>'."""
    return [os.path.join(out_dir, 'pred_' + os.path.basename(l[0])[:-(len(ending) + 5)]) for l in lists]


def main():
    doc = {'folders': FOLDERS, 'existing': EXISTING, 'lists': [], 'manage': []}
    with tempfile.TemporaryDirectory() as root:
        for name, files in FOLDERS.items():
            make_folder(root, name, files)
        for name, ending in LIST_CASES:
            res = create_lists_from_splitted_dataset_folder(os.path.join(root, name), ending)
            doc['lists'].append({'folder': name, 'ending': ending, 'result': relative(res, root)})
        for n, case in enumerate(MANAGE_CASES):
            src = os.path.join(root, case['src'])
            out_files = [('pred_' if case['output'] == 'list' else '') + f for f in EXISTING[case['existing']]]
            out_dir = make_folder(root, f'out_{n}', out_files)
            lists = create_lists_from_splitted_dataset_folder(src, case['ending'])
            source = src if case['source'] == 'folder' else lists
            output = {'folder': out_dir, 'list': truncated_list(lists, case['ending'], out_dir), None: None}[case['output']]
            stand_in = types.SimpleNamespace(dataset_json={'file_ending': case['ending']})
            res = nnUNetPredictor._manage_input_and_output_lists(
                stand_in, source, output, os.path.join(root, 'prev') if case['prev'] else None, case['overwrite'],
                case['part_id'], case['num_parts'], case['save_probabilities'])
            doc['manage'].append({**case, 'out_dir': f'out_{n}', 'out_files': out_files, 'source_arg': relative(source, root),
                                  'output_arg': relative(output, root), 'result': relative([list(r) if r is not None else None for r in res], root)})
    with open(os.path.join(HERE, 'imageio.json'), 'w') as f:
        json.dump(doc, f, indent=1)
    print('imageio', len(doc['lists']), 'list cases,', len(doc['manage']), 'manage cases')


if __name__ == '__main__':
    main()

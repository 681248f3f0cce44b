"""Projection of every selected slice of every patient volume (SG3/genlib/projector/projection_loop.py, control flow
restated, quirks included):

  * the dataset is walked in file order, batch 1, unshuffled; only every `step_patient_slice`-th ITEM is projected
    (the counter runs over the whole dataset, not per patient);
  * the first projected slice of a patient runs cold (w from the generator's mean) with its own step count and no
    early stopping;
  * every later slice of that patient starts from THAT FIRST slice's best w -- the reference does not advance the
    start slice by slice;
  * the result is pickled to run_dir/projected_w as {patient: {slice: w [num_ws, w_dim]}} (plain dicts).

Differences from the reference by design:
  * the device is cuda:<rank> (the reference hard-codes cuda:1);
  * the cold start's 1000 steps / patience 100000 are projector_kwargs.first_num_steps / first_early_stopping with
    those defaults;
  * projection_test passes num_steps and early_stopping from projector_kwargs (the reference's call omits the two
    required arguments and cannot run);
  * projector_kwargs.class_name, when present, names the projector class to construct (default: this package's);
  * projector_kwargs.batch > 1 projects `batch` slices at a time (_project_batched): the same slices from the same
    starts, first all cold first slices, then all warm ones; at 1 (the default) the loop below runs as it always did.
"""
import os
import pickle

import numpy as np
import torch

import dnnlib
from genlib.utils import util_general

PROJECTOR_CLASS = 'genlib.projector.projector.StyleGAN2Projector'
FIRST_NUM_STEPS, FIRST_EARLY_STOPPING = 1000, 100000


def _device(rank):
    return torch.device('cuda', rank)


def _seed(random_seed, num_gpus, rank, cudnn_benchmark):
    np.random.seed(random_seed * num_gpus + rank)
    torch.manual_seed(random_seed * num_gpus + rank)
    torch.backends.cudnn.benchmark = cudnn_benchmark
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False


def projection_loop(run_dir='.', training_set_kwargs={}, projector_kwargs={}, random_seed=0, num_gpus=1, rank=0,
                    batch_size=1, image_snapshot_ticks=50, network_snapshot_ticks=50, cudnn_benchmark=True):
    device = _device(rank)
    _seed(random_seed, num_gpus, rank, cudnn_benchmark)
    training_set_kwargs = dnnlib.EasyDict(training_set_kwargs)
    projector_kwargs = dnnlib.EasyDict(projector_kwargs)

    print('Loading training set...')
    training_set = dnnlib.util.construct_class_by_name(**training_set_kwargs)
    loader = torch.utils.data.DataLoader(dataset=training_set, batch_size=batch_size // num_gpus, shuffle=False)
    print()
    print('Num images: ', len(training_set))
    print('Image shape:', training_set.image_shape)
    print('Label shape:', training_set.label_shape)
    print()

    if rank == 0:
        print('Constructing Projector...')
    projector = dnnlib.util.construct_class_by_name(
        class_name=projector_kwargs.get('class_name', PROJECTOR_CLASS), outdir=run_dir, device=device,
        modalities=training_set_kwargs.modalities, dtype=training_set_kwargs.dtype,
        **{k: v for k, v in projector_kwargs.items() if k != 'class_name'})

    first_num_steps = projector_kwargs.get('first_num_steps', FIRST_NUM_STEPS)
    first_early_stopping = projector_kwargs.get('first_early_stopping', FIRST_EARLY_STOPPING)
    if int(projector_kwargs.get('batch', 1)) > 1:
        projected_w = _project_batched(loader, projector, projector_kwargs, device, first_num_steps, first_early_stopping)
        _dump(run_dir, projected_w)
        return
    projected_w = util_general.nested_dict()
    current_patient, w_init = '', None
    for idx, (image, _label, fname) in enumerate(loader):
        if idx % projector_kwargs.step_patient_slice != 0:
            continue
        image = image.to(device).to(torch.float32)          # [1, modalities, H, W]
        _, id_patient, id_slice = util_general.split_dos_path_into_components(path=fname[0])
        id_slice = util_general.get_filename_without_extension(path=id_slice)[-5:]
        print(f'Patient:        {id_patient}')
        print(f'Slice:          {id_slice}')
        print('')
        if id_patient == current_patient:       # warm start from the patient's first projected slice
            assert w_init is not None
            w_steps, best_step = projector.forward(
                id_patient=id_patient, id_slice=int(id_slice), target=image, num_steps=projector_kwargs.num_steps,
                early_stopping=projector_kwargs.early_stopping, w_init=w_init, verbose=projector_kwargs.verbose)
        else:
            w_steps, best_step = projector.forward(
                id_patient=id_patient, id_slice=int(id_slice), target=image, num_steps=first_num_steps,
                early_stopping=first_early_stopping, verbose=False)
            current_patient = id_patient
            w_init = w_steps[best_step].detach().cpu()
        projected_w[id_patient][id_slice] = w_steps[best_step].detach().cpu().numpy()
    _dump(run_dir, projected_w)


def _dump(run_dir, projected_w):
    with open(os.path.join(run_dir, 'projected_w'), 'wb') as handle:
        pickle.dump(util_general.plain_dict(projected_w), handle, protocol=pickle.HIGHEST_PROTOCOL)


def _selected(loader, step_patient_slice):
    """The items the sequential loop projects, in dataset order: (group, first of its group, id_patient, id_slice,
    image [1, modalities, H, W]).  A group is a run of consecutive selected items of one patient -- the sequential
    loop's comparison with the previous selected item's patient."""
    current_patient, group = '', -1
    for idx, (image, _label, fname) in enumerate(loader):
        if idx % step_patient_slice != 0:
            continue
        _, id_patient, id_slice = util_general.split_dos_path_into_components(path=fname[0])
        id_slice = util_general.get_filename_without_extension(path=id_slice)[-5:]
        first = id_patient != current_patient
        if first:
            current_patient, group = id_patient, group + 1
        yield group, first, id_patient, id_slice, image


def _project_batched(loader, projector, projector_kwargs, device, first_num_steps, first_early_stopping):
    """projector_kwargs.batch > 1: the same slices from the same starts as the sequential loop, `batch` at a time
    (projector.forward_batch).  Every warm slice starts from its own group's FIRST slice's best w, so all warm slices
    are independent of one another, and so are all cold first slices:
      phase A: the first slice of every group, cold (first_num_steps / first_early_stopping, not verbose), in dataset
               order, `batch` at a time;
      phase B: every other selected slice, warm from its group's first best w (a per-sample w_init), in dataset order,
               `batch` at a time -- a batch may mix patients.
    The last batch of a phase may be short.  The dataset is walked once per phase, so at most `batch` images are held.
    Returns {patient: {slice: w}} with the keys in dataset order, as the sequential loop leaves them."""
    batch = int(projector_kwargs.batch)
    projected_w = util_general.nested_dict()
    group_w = {}                # group -> its first slice's best w [num_ws, w_dim] (CPU)

    def flush(pending, warm):
        if not pending:
            return
        for _, id_patient, id_slice, _ in pending:
            print(f'Patient:        {id_patient}')
            print(f'Slice:          {id_slice}')
        print('')
        ids = [(id_patient, int(id_slice)) for _, id_patient, id_slice, _ in pending]
        targets = torch.cat([image for _, _, _, image in pending]).to(device).to(torch.float32)
        if warm:
            w_steps, best_steps = projector.forward_batch(
                ids=ids, targets=targets, num_steps=projector_kwargs.num_steps,
                early_stopping=projector_kwargs.early_stopping, w_init=torch.stack([group_w[g] for g, _, _, _ in pending]),
                verbose=projector_kwargs.verbose)
        else:
            w_steps, best_steps = projector.forward_batch(
                ids=ids, targets=targets, num_steps=first_num_steps, early_stopping=first_early_stopping, verbose=False)
        for b, (group, id_patient, id_slice, _) in enumerate(pending):
            best = w_steps[b][int(best_steps[b])].detach().cpu()
            if not warm:
                group_w[group] = best
            projected_w[id_patient][id_slice] = best.numpy()
        pending.clear()

    for warm in (False, True):
        pending = []
        for group, first, id_patient, id_slice, image in _selected(loader, projector_kwargs.step_patient_slice):
            if not warm:
                projected_w[id_patient][id_slice] = None        # the keys in dataset order
            if first == warm:
                continue
            pending.append((group, id_patient, id_slice, image))
            if len(pending) == batch:
                flush(pending, warm)
        flush(pending, warm)
    return projected_w


def projection_test(target_fname='.', run_dir='.', training_set_kwargs={}, projector_kwargs={}, random_seed=0,
                    num_gpus=1, rank=0, cudnn_benchmark=True):
    """Project one image file named <patient>_<slice>.<ext> (grey, 256 x 256 as the reference reshapes it)."""
    from PIL import Image
    device = _device(rank)
    _seed(random_seed, num_gpus, rank, cudnn_benchmark)
    print('Loading Test Image...')
    pil = Image.open(target_fname)
    if pil.format != 'TIFF':
        pil = pil.convert('L')
    array = np.array(pil)
    if array.max() <= 1:
        print(f'Unsupported max value : Expected values in [0, 255] but got [{array.min()}, {array.max()}]!')
        array = array * 255.0
    target = torch.Tensor(array)
    if target.ndim != 4:
        print(f'Unsupported input dimension: Expected 4D (batched) input but got input of size: {target.shape}! '
              f'Let\'s add dimension!')
        target = target.view([1, 1, 256, 256])
    if target.dtype != torch.float32:
        target = target.to(torch.float32)
    print()
    print('Image shape:', target.shape)
    print('Image dtype:', target.dtype)
    print('Image min:', target.min().item())
    print('Image max:', target.max().item())
    print()

    if rank == 0:
        print('Constructing Projector...')
    projector_kwargs = dnnlib.EasyDict(projector_kwargs)
    projector = dnnlib.util.construct_class_by_name(
        class_name=projector_kwargs.get('class_name', PROJECTOR_CLASS), outdir=run_dir, device=device,
        modalities=training_set_kwargs['modalities'], dtype=training_set_kwargs['dtype'],
        **{k: v for k, v in projector_kwargs.items() if k != 'class_name'})
    idp, ids = util_general.get_filename_without_extension(target_fname).split('_')
    return projector.forward(id_patient=idp, id_slice=int(ids), target=target, num_steps=projector_kwargs.num_steps,
                             early_stopping=projector_kwargs.early_stopping, verbose=True)

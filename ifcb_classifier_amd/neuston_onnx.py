"""Twin of the reference's ``neuston_onnx.py``: ``EXPORT`` a trained ``.ptl`` to ``.onnx`` + ``.classes``, ``RUN`` an ``.onnx``
on images.  Same command line.

EXPORT reads the checkpoint with the tolerant unpickler and writes the file with ``onnx_export`` (no ``onnx`` package, no
engine, no GPU).  RUN of a file this package wrote (``ifcbk.*`` metadata) rebuilds the backbone and classifies on the GPU
through the engine's eval forward and softmax; any other ``.onnx`` goes to ``onnxruntime`` as upstream does.

    python -m ifcb_classifier_amd.neuston_onnx EXPORT MODEL.ptl [--half] [--opset 12] [--batchsize 0] [--output PATH]
    python -m ifcb_classifier_amd.neuston_onnx RUN MODEL.onnx SRC [--classfile CLASSES]
"""
import argparse
import os

import numpy as np
import torch

from . import onnx_export
from .neuston_data import IMG_EXTENSIONS

RUN_BATCH = 32


def do_export(args):
    from .neuston_models import load_checkpoint_file
    ckpt = load_checkpoint_file(args.MODEL)
    hp = dict(ckpt['hyper_parameters'])
    classes = list(hp['classes'])
    if args.output:
        output = args.output
        os.makedirs(os.path.dirname(output) or '.', exist_ok=True)
    else:
        output = args.MODEL.replace('.ptl', '.onnx')
        if args.half:
            output = output.replace('.onnx', '.FP16.onnx')
    print(hp['MODEL'])
    # (--device is accepted for upstream's command line: the file is written from the checkpoint's tensors on the host)
    onnx_export.export(ckpt['state_dict'], hp['MODEL'], classes, hp.get('pretrained', False), output, half=args.half,
                       opset=args.opset, batch_size=args.batchsize, pad=hp.get('pad'))
    print('EXPORTED:', output)
    output_classes = output.replace('.onnx', '.classes')
    onnx_export.write_classes(output_classes, classes)
    print('EXPORTED:', output_classes)
    return output, output_classes


def collect_images(src):
    """upstream's inputs: a directory (walked recursively), a .txt / .list file of paths, or one image"""
    img_paths = []
    if os.path.isdir(src):
        for pardir, _, imgs in os.walk(src):
            img_paths.extend(os.path.join(pardir, img) for img in imgs if img.endswith(IMG_EXTENSIONS))
    elif os.path.isfile(src) and src.endswith(('.txt', '.list')):
        with open(src) as f:
            img_paths = [img.strip() for img in f.read().splitlines()]
        img_paths = [img for img in img_paths if img.endswith(IMG_EXTENSIONS)]
    elif src.endswith(IMG_EXTENSIONS):
        img_paths.append(src)
    return img_paths


def load_backbone(model, precision='bf16', max_batch=RUN_BATCH, device=0):
    """a ``NeustonModel`` rebuilt from an ``.onnx`` this package wrote: backbone from the ``ifcbk.*`` metadata, weights from the
    initializers (float16 files upcast).  Returns (NeustonModel, resize)."""
    from .neuston_models import NeustonModel
    meta = model['metadata']
    nc = int(meta['ifcbk.num_classes'])
    hp = argparse.Namespace(MODEL=meta['ifcbk.model'], classes=[str(i) for i in range(nc)],
                            pretrained=meta['ifcbk.pretrained'] == '1', precision=precision, batch_size=max_batch)
    classifier = NeustonModel(hp, device=device, max_batch=max_batch, train_batch=1)
    sd = classifier.model.state_dict()
    inits = {k: v for k, v in model['initializers'].items() if not k.startswith('transform_input.')}
    unknown = [k for k in inits if k not in sd]
    if unknown:
        raise ValueError('initializers %s are not tensors of %s' % (unknown[:5], hp.MODEL))
    for k, v in inits.items():
        if tuple(v.shape) != tuple(sd[k].shape):
            raise ValueError('initializer %s has shape %s, %s expects %s' % (k, v.shape, hp.MODEL, tuple(sd[k].shape)))
        sd[k] = torch.from_numpy(v.astype(np.float32))
    classifier.model.load_state_dict(sd)
    return classifier, int(meta['ifcbk.resize'])


def classify(classifier, dataset, batch_size=RUN_BATCH):
    """eval forward + softmax of every image of ``dataset`` (an ``ImageDataset``) on the GPU: (logits, probs) numpy arrays"""
    from torch.utils.data import DataLoader
    from .neuston_data import collate_rois
    loader = DataLoader(dataset, batch_size=batch_size, shuffle=False, num_workers=0, collate_fn=collate_rois)
    head = classifier.model._train_heads[0]
    logits, probs = [], []
    for rois, _ in loader:
        n = classifier.stage_batch(rois, dataset.transform)
        classifier.use_staged()
        p, _ = classifier.eval_current(n)
        logits.append(head.logits[:n].float().cpu())
        probs.append(p.float().cpu())
    return torch.cat(logits).numpy(), torch.cat(probs).numpy()


def _host_tensor(img, resize):
    """Resize([resize, resize]) + ToTensor on the host, for a runtime that takes the CHW float array"""
    from PIL import Image
    im = Image.fromarray(img).convert('RGB').resize((resize, resize), Image.BILINEAR)
    return np.asarray(im, np.float32).transpose(2, 0, 1) / 255


def do_run(args):
    from .neuston_data import ImageDataset
    img_paths = collect_images(args.SRC)
    model = onnx_export.read(args.MODEL)
    if 'ifcbk.model' in model['metadata']:
        classifier, resize = load_backbone(model, args.precision, device=int(os.environ.get('LOCAL_RANK', 0)))
        image_dataset = ImageDataset(img_paths, resize=resize, input_src=args.SRC, pad=onnx_export.read_pad(model['metadata']))
        logits, out = classify(classifier, image_dataset)
    else:
        try:
            import onnxruntime as ort
        except ImportError:
            raise SystemExit('RUN: %s was not exported by ifcb_classifier_amd (no ifcbk.* metadata); running a foreign ONNX '
                             'file needs the onnxruntime package, which is not installed' % args.MODEL)
        from scipy.special import softmax
        inp = model['inputs'][0]
        resize = inp['dims'][-1] if isinstance(inp['dims'][-1], int) else 299
        image_dataset = ImageDataset(img_paths, resize=resize, input_src=args.SRC)
        dt = np.float16 if inp['elem_type'] == onnx_export.FLOAT16 else np.float32
        input_array = np.asarray([_host_tensor(img, resize) for (img, _), _ in image_dataset], dt)
        logits = np.asarray(ort.InferenceSession(args.MODEL).run(None, {inp['name']: input_array})[0])
        out = softmax(logits.astype(np.float32), axis=1)
    output_classes = np.argmax(out, axis=1)
    output_scores = np.max(out, axis=1)
    print(output_scores)
    print(output_classes)
    classfile = args.classfile or args.MODEL.replace('.onnx', '.classes')
    print(classfile)
    labels = None
    if os.path.isfile(classfile):
        with open(classfile) as f:
            classes = f.read().splitlines()
        labels = [classes[idx] for idx in output_classes]
        print(labels)
    return dict(images=image_dataset.image_paths, logits=logits, probs=out, labels=labels)


def argparse_onnx():
    parser = argparse.ArgumentParser(description='Convert ptl models to ONNX')
    subparsers = parser.add_subparsers(dest='cmd_mode', help='These sub-commands are mutually exclusive.')
    export = subparsers.add_parser('EXPORT', help='Export a .ptl model to .onnx')
    run = subparsers.add_parser('RUN', help='Run an onnx model')

    export.add_argument('MODEL', help='Model .ptl file to convert')
    export.add_argument('--half', action='store_true', help='Exports model using 16bit floating point precision')
    export.add_argument('--device', default='cpu', choices=('cpu', 'cuda'), help='Accepted for upstream\'s command line; the export reads the checkpoint on the host either way')
    export.add_argument('--opset', default=12, type=int, help='Opset Version for onnx. Default is 12.')
    export.add_argument('--batchsize', default=0, type=int, help='Set a fixed batch input/output batch size for the model. Default is None, ie dynamic batch size')
    export.add_argument('--output', default=None, help='Same as model file but with ".ptl" replaced with ".onnx"')

    run.add_argument('MODEL', help='onnx model file')
    run.add_argument('SRC', help='file to run the model on')
    run.add_argument('--classfile', '-c', help='file with list of class labels')
    run.add_argument('--precision', choices=['bf16', 'fp32'], default='bf16', help='(MI355X path, additive) activation storage / MFMA type for files exported by this package, as neuston_net --precision. Default is bf16')
    return parser


def main(argv=None):
    args = argparse_onnx().parse_args(argv)
    if args.cmd_mode == 'EXPORT':
        return do_export(args)
    return do_run(args)


if __name__ == '__main__':
    main()

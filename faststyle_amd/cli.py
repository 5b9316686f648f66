"""Command-line surfaces of the drop-in scripts.  The FLAG NAMES, DEFAULTS, TYPES and CHOICES are the
reference's interface (stylize_image.py:19-43, train.py:23-105, slow_style.py:17-67,
stylize_webcam.py:17-39) and are kept exactly -- tests/test_scripts.py and tests/test_aux_scripts.py
pin them; the help texts are this project's own."""
import argparse

LAYERS_STYLE = ['conv1_2', 'conv2_2', 'conv3_3', 'conv4_3']
UPSAMPLE = dict(choices=['resize', 'deconv'], default='resize',
                help="how the model's two upsampling layers were built: 'resize' (nearest x4 + stride-2 conv, the shipped "
                     "models) or 'deconv' (conv2d_transpose); a mismatch with the checkpoint is an error")

LOSS_FLAGS = [
    ('--loss_content_layers', dict(nargs='*', default=['conv3_3'], help='VGG16 layers of the content loss')),
    ('--loss_style_layers', dict(nargs='*', default=LAYERS_STYLE, help='VGG16 layers whose Gram matrices define the style loss')),
    ('--content_weights', dict(nargs='*', default=[1.0], type=float, help='one weight per content layer')),
    ('--style_weights', dict(nargs='*', default=[5.0, 5.0, 5.0, 5.0], type=float, help='one weight per style layer')),
]


def _build(description, flags):
    parser = argparse.ArgumentParser(description=description)
    for name, kw in flags:
        parser.add_argument(name, **kw)
    return parser


def stylize_image_parser():
    return _build("Filter one image through a trained transform net (HIP engine on MI355X).", [
        ('--input_img_path', dict(help='image to stylize')),
        ('--output_img_path', dict(default='./results/styled.jpg', help='where the result is written')),
        ('--model_path', dict(default='./models/starry_final.ckpt', help='checkpoint prefix of the trained net (bundle V2)')),
        ('--content_target_resize', dict(default=1.0, type=float, help='scale factor applied to the input first')),
        ('--upsample_method', dict(UPSAMPLE)),
    ])


def train_parser():
    return _build("Train a transform net against the VGG16 perceptual loss (HIP engine, optionally data-parallel).", [
        ('--train_dir', dict(help="directory of train-* TFRecord shards (or of image files, or the literal 'synthetic')")),
        ('--model_name', dict(help='name used for checkpoints, the final model and the default log directory')),
        ('--style_img_path', dict(default='./style_images/starry_night_crop.jpg', help='style target image')),
        ('--learn_rate', dict(default=1e-3, type=float, help='Adam step size')),
        ('--batch_size', dict(default=4, type=int, help='images per step (per GPU when launched data-parallel)')),
        ('--n_epochs', dict(default=2, type=int, help='passes over the training set')),
        ('--preprocess_size', dict(default=[256, 256], nargs=2, type=int, help='training images are resized to H W')),
        ('--run_name', dict(default=None, help='log sub-directory under ./summaries/train (default: <model_name><k>)')),
    ] + LOSS_FLAGS + [
        ('--num_steps_ckpt', dict(default=1000, type=int, help='checkpoint period in steps')),
        ('--num_pipe_buffer', dict(default=4000, type=int, help='images held by the shuffle queue (min_after_dequeue)')),
        ('--num_steps_break', dict(default=-1, type=int, help='stop after this step (-1: run all epochs)')),
        ('--resume_from', dict(default=None, help='bundle prefix of a training/<model_name>.ckpt-<step> to continue from '
                                             '(weights, Adam slots, global_step); not in the reference')),
        ('--no_graph', dict(action='store_true', help='launch every kernel of a step eagerly instead of replaying the captured '
                                                      'hipGraph (the default, and what bench.py times); not in the reference')),
        ('--beta', dict(default=0.0, type=float, help='total-variation weight (about 1e-4 helps deconv models)')),
        ('--style_target_resize', dict(default=1.0, type=float, help='scale factor applied to the style image')),
        ('--upsample_method', dict(UPSAMPLE)),
    ])


def slow_style_parser():
    return _build("Optimise the pixels of an image against the perceptual loss (Gatys et al.), VGG16 variant.", [
        ('--style_img_path', dict(help='style image')),
        ('--cont_img_path', dict(help='content image')),
        ('--learn_rate', dict(default=1e1, type=float, help='Adam step size on the 0..255 pixel scale')),
    ] + LOSS_FLAGS + [
        ('--num_steps_break', dict(default=500, type=int, help='optimiser iterations')),
        ('--beta', dict(default=1.e-4, type=float, help='total-variation weight')),
        ('--style_target_resize', dict(default=1.0, type=float, help='scale factor applied to the style image')),
        ('--cont_target_resize', dict(default=1.0, type=float, help='scale factor applied to the content image (= output size)')),
        ('--output_img_path', dict(default='./out.jpg', help='where the result is written')),
    ])


def stylize_webcam_parser():
    return _build("Filter a webcam feed (or a directory of frames) through a trained transform net.", [
        ('--model_path', dict(default='./models/starry_final.ckpt', help='checkpoint prefix of the trained net')),
        ('--upsample_method', dict(UPSAMPLE)),
        ('--resolution', dict(nargs=2, type=int, default=None, help='capture width height (default: the camera default)')),
        ('--frames_dir', dict(default=None, help='(addition) read frames from this directory instead of a camera')),
        ('--output_dir', dict(default='./frames_out', help='(addition) where --frames_dir results go')),
        ('--output_format', dict(choices=['png', 'jpg'], default='png', help="(addition) file type of the --frames_dir results: 'png' through PIL, "
                                                                            "'jpg' encoded by the library (forward DCT on the GPU, 4:2:0)")),
        ('--output_quality', dict(default=95, type=int, help='(addition) JPEG quality 1..100 of --output_format jpg')),
        ('--frame_size', dict(nargs=2, type=int, default=None, metavar=('W', 'H'),
                              help="(addition) resize every --frames_dir frame to W x H on the device with cv2.resize's resampling (area when "
                                   "shrinking, cubic otherwise); not together with --resolution, which keeps its PIL resize; also resizes "
                                   "--video_in frames")),
        ('--input_decode', dict(choices=['pil', 'native'], default='pil',
                                help="(addition) decoder of the --frames_dir frames: 'pil', or 'native' -- baseline .jpg / .jpeg files go in as "
                                     "bytes (Huffman pass on host threads, reconstruction on the GPU); other files still go through PIL")),
        ('--video_in', dict(default=None, metavar='PATH|-',
                            help="(addition) read frames from this YUV4MPEG2 stream ('-': standard input), e.g. the output of ffmpeg -f yuv4mpegpipe; "
                                 "colour conversion on the device; composes with --frame_size, not with --frames_dir or --resolution")),
        ('--video_out', dict(default=None, metavar='PATH|-',
                             help="(addition) write the --video_in results as a YUV4MPEG2 stream ('-': standard output, every message then goes to "
                                  "standard error) with the input's frame rate, aspect, sampling, siting and range; without it they go to --output_dir")),
        ('--video_matrix', dict(choices=['bt601', 'bt709'], default='bt601',
                                help="(addition) YCbCr matrix of the --video_in / --video_out streams (the format does not record it)")),
        ('--video_depth', dict(choices=['8', 'stream'], default='8',
                               help="(addition) bits per sample taken from --video_in: '8' refuses deeper streams (C420p10 ...), 'stream' takes the "
                                    "stream's own depth, 8 to 16 bits, and feeds 9 to 16 bits to the net without a u8 stage; not with --frame_size")),
        ('--video_out_depth', dict(default=None, type=int, choices=list(range(8, 17)), metavar='N',
                                   help="(addition) bits per sample of --video_out, 8..16 (default: the input's); above 8 the net's fp32 output "
                                        "goes to the planes without a u8 stage")),
        ('--style_strength', dict(default=None, type=float, metavar='S',
                                  help="(addition) blend every stylized frame back towards its source on the device: 0 the source, 1 the net's "
                                       "output (default: no such stage); with --frames_dir, --video_in and the camera, every input and output flag")),
        ('--preserve_color', dict(action='store_true',
                                  help="(addition) keep the source's colours and take the stylized luminance only (alone: at strength 1)")),
        ('--color_matrix', dict(choices=['bt601', 'bt709'], default=None,
                                help="(addition) luma weights of --preserve_color (default: --video_matrix with --video_in, else bt601)")),
        ('--mask_path', dict(default=None, metavar='FILE',
                             help="(addition) a grey image of the net's input size (after --frame_size): 0 keeps the source pixel, 255 stylizes it, "
                                  "values between blend")),
        ('--temporal_strength', dict(default=argparse.SUPPRESS, type=float, metavar='S',
                                     help="(addition) stabilise the frames over time on the device: blend every frame towards the previous stabilised "
                                          "frame, fetched along block motion vectors, where the source matched; 0 nothing, 1 all of it (default: no "
                                          "such stage); with --frames_dir, --video_in and the camera")),
        ('--temporal_radius', dict(default=argparse.SUPPRESS, type=int, metavar='R', help="(addition) search radius of the motion vectors in pixels, 0..7 (default 7)")),
        ('--temporal_levels', dict(default=argparse.SUPPRESS, type=int, metavar='L',
                                   help="(addition) search the motion vectors coarse to fine over L halved lumas, 1..3 (default 1): fast motion, "
                                        "found reliably up to about R 2^(L-1) pixels; needs --temporal_strength")),
        ('--temporal_subpel', dict(default=argparse.SUPPRESS, type=int, metavar='S',
                                   help="(addition) motion vectors in whole (0, the default), half (1) or quarter pixels (2): slow motion keeps "
                                        "its match, for one more launch and a bilinear fetch; needs --temporal_strength")),
        ('--temporal_overlap', dict(default=argparse.SUPPRESS, type=int, metavar='O',
                                    help="(addition) 1: blend every pixel along the vectors of the four blocks around it, weighted by a window and "
                                         "by how well each matched, so that motion edges inside a block keep their match; 0 (the default): whole "
                                         "blocks; needs --temporal_strength")),
        ('--temporal_sensitivity', dict(default=argparse.SUPPRESS, type=int, metavar='K',
                                        help="(addition) how fast a source mismatch turns the blend off, 1..256: none of it is left at a luma "
                                             "difference of 256 / K (default 16)")),
        ('--output_size', dict(default=argparse.SUPPRESS, nargs='+', metavar='W H|source',
                               help="(addition) deliver every frame at W x H, or with 'source' at the stream's or first frame's own size, whatever "
                                    "size the net runs at (--frame_size): Pillow's mode-F resampling of the net's fp32 output on the device, ahead of "
                                    "every output conversion; with --frames_dir, --video_in and the camera")),
        ('--output_filter', dict(default=argparse.SUPPRESS, choices=['box', 'bilinear', 'bicubic', 'lanczos'], metavar='F',
                                 help="(addition) filter of --output_size: box, bilinear, bicubic (default) or lanczos")),
        ('--output_guided', dict(default=argparse.SUPPRESS, action='store_true',
                                 help="(addition) with --frame_size and an --output_size that is the source's: deliver by edge-aware (guided) "
                                      "upsampling against the full-size source instead of a resampling filter, so that the source's edges return "
                                      "at the delivery resolution; with --frames_dir, --video_in and the camera")),
        ('--guided_radius', dict(default=argparse.SUPPRESS, type=int, metavar='R',
                                 help="(addition) window radius of --output_guided on the net's grid, 1..8 (default 2)")),
        ('--guided_smoothness', dict(default=argparse.SUPPRESS, type=int, metavar='E',
                                     help="(addition) smoothness of --output_guided in 8-bit levels, 1..64 (default 4): larger follows the source's "
                                          "edges less")),
        ('--video_batch', dict(default=argparse.SUPPRESS, type=int, metavar='N',
                               help="(addition) with --video_in: N consecutive frames per pass through the net, 1..64 (default 1); with "
                                    "--temporal_strength the stage runs over the N frames in order; the results are written in order, a stream's "
                                    "last frames included; latency grows by N frames, so live pipes keep 1")),
        ('--video_also', dict(default=argparse.SUPPRESS, action='append', nargs=2, metavar=('IN', 'OUT'),
                              help="(addition) with --video_in and --video_out, repeatable (up to 63 times): one more YUV4MPEG2 stream of the same "
                                   "size and format, stylized in the same passes -- a batch across streams, which costs no latency; with "
                                   "--temporal_strength every stream is stabilised on its own; not with --video_batch")),
        ('--precision', dict(default=argparse.SUPPRESS, choices=['fp32', 'bf16'],
                             help="(addition) arithmetic of the net: fp32 (default) or bf16, the mixed-precision path of resize-conv models "
                                  "(about twice the frame rate, about 52 dB against fp32; not with --upsample_method deconv); with --frames_dir, "
                                  "--video_in and the camera")),
        ('--frame_filter', dict(default=argparse.SUPPRESS, choices=['box', 'bilinear', 'bicubic', 'lanczos'], metavar='F',
                                help="(addition) with --video_depth stream, a --video_in of 9 to 16 bits and --frame_size: resample the stream's fp32 "
                                     "frames to W x H with this filter on the device (without it --frame_size refuses such a stream)")),
        ('--model_path2', dict(default=argparse.SUPPRESS, metavar='CKPT',
                               help="(addition) checkpoint prefix of a second trained net (same --upsample_method): every frame goes through both "
                                    "and the two fp32 outputs are mixed on the device ahead of every later stage; needs --style_mix, --mix_mask or "
                                    "--mix_fade; with --frames_dir, --video_in and the camera")),
        ('--style_mix', dict(default=argparse.SUPPRESS, type=float, metavar='T',
                             help="(addition) share of the second model, 0..1 (default 1): 0 shows --model_path, 1 --model_path2; a model nobody "
                                  "will see is not run")),
        ('--mix_mask', dict(default=argparse.SUPPRESS, metavar='FILE',
                            help="(addition) a grey image of the net's input size (after --frame_size): 0 shows --model_path at that pixel, 255 "
                                 "the mix, values between blend")),
        ('--mix_fade', dict(default=argparse.SUPPRESS, nargs=2, type=int, metavar=('F0', 'F1'),
                            help="(addition) cross-fade: the share of the second model rises from 0 at frame F0 to --style_mix at frame F1 "
                                 "(0-based, 0 <= F0 < F1); with --frames_dir and --video_in")),
    ])

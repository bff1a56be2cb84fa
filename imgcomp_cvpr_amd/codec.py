"""Image codec: an image to a self-describing file and back.

    python -m imgcomp_cvpr_amd.codec compress   IN.png  OUT.icf [--ae_config cvpr/low] [--pc_config cvpr/res_shallow] [--weights synthetic|FILE.npz|CKPT]
                                                                [--tile PIXELS [--checked | --wavefront | --layers a,b,.. | --progressive |
                                                                                --front-layers a,b,.. | --front-progressive |
                                                                                --depth [--depth-block B] | --rans [--lanes W]]]
                                                                [--cap T | --max-bytes N | --bpp B | --min-psnr D | --min-ms-ssim S]
                                                                [--roi X,Y,W,H ... [--background T]] [--rdo LAMBDA]
    python -m imgcomp_cvpr_amd.codec decompress IN.icf  OUT.png [same options] [--salvage | --channels K | --partial | --recover]
    python -m imgcomp_cvpr_amd.codec decompress IN.icf  OUT.png [same options] --region X,Y,W,H [--channels K]    a rectangle, from the tiles it needs
    python -m imgcomp_cvpr_amd.codec info PATH [PATH ...] [--region X,Y,W,H]    what the files hold and what a region would decode, without model or device
    python -m imgcomp_cvpr_amd.codec compress-dir   IN_DIR OUT_DIR [--tile PIXELS [same choices]] [--batch N] [--cap T | --max-bytes N | --bpp B] [--rdo LAMBDA]   every *.png / *.jpg -> OUT_DIR/<stem>.icf
    python -m imgcomp_cvpr_amd.codec decompress-dir IN_DIR OUT_DIR [--batch N] [--salvage | --channels K | --partial | --recover]    every *.icf -> OUT_DIR/<stem>.png
    python -m imgcomp_cvpr_amd.codec verify PATH [PATH ...]         files or directories of *.icf: the checksums, without model or device
    python -m imgcomp_cvpr_amd.codec stream IN.icf OUT_DIR [model options] [--chunk BYTES]    a format-6 file fed chunk by chunk, a picture per gained layer
    python -m imgcomp_cvpr_amd.codec stream IN.icf OUT_DIR --fronts [model options] [--chunk BYTES]    the same for a format-6 or a format-8 file
    python -m imgcomp_cvpr_amd.codec transcode IN.icf OUT.icf [model options] [--tile PIXELS [the choices of compress]]
                                                              [--cap K | --max-bytes N | --bpp B] [--roi X,Y,W,H ... [--background K]] [--salvage | --recover]
                                                              [--min-psnr D | --min-ms-ssim S]    against the picture IN.icf decodes to
    python -m imgcomp_cvpr_amd.codec transcode-dir IN_DIR OUT_DIR [the same, without --roi] [--batch N]     every *.icf -> OUT_DIR/<stem>.icf
    python -m imgcomp_cvpr_amd.codec measure IN.png IN.icf [model options] [--channels K] [--region X,Y,W,H]    bytes, bpp, PSNR, MS-SSIM of the file
    python -m imgcomp_cvpr_amd.codec rd IN.png OUT.json [model options] [--tile PIXELS [the choices of compress]] [--levels N] [--roi X,Y,W,H ...]
                                                              the rate-distortion table of the cap levels k C / N as JSON, a line per level
    python -m imgcomp_cvpr_amd.codec rd IN.png OUT.json [model options] [--tile PIXELS [the choices of compress]] --rdo-levels a,b,..
                                                              the same table over lambdas of --rdo in place of cap levels

compress:   pad to a multiple of the subsampling factor (val.add_padding) -> ae.encode -> PredictionNetwork.encode_stream (the
            range coder on the device, ic_pc_encode_f32) -> container.
decompress: parse + check the container -> PredictionNetwork.decode_stream (ic_pc_decode_f32) -> centers[symbols] -> ae.decode ->
            truncating cast to uint8 (as val.py) -> crop the padding away.
The payload is the coder's byte stream, unchanged: 8 * len(payload) is the number val.py --real_bpp reports for the image.

Container (little-endian; INTEGRATION.md has the same table):
    offset  size  field
    0       4     magic  b'ICVF'
    4       2     format version (u16) = 1
    6       2+a   ae config name: length a (u16), then a bytes of UTF-8
    ..      2+p   pc config name: length p (u16), then p bytes of UTF-8
    ..      4+4   original image H, W (u32, u32)
    ..      2+4+4 symbol volume C (u16), h, w (u32, u32)
    ..      2     L, the number of centres (u16)
    ..      2     first_sym, the uncoded first symbol (u16)
    ..      8     frequency resolution of the coder's tables (f64)
    ..      4     model fingerprint (u32): CRC-32 over the centres and the context-model weights
    ..      8     payload length n (u64)
    ..      n     payload
    ..      4     CRC-32 (zlib.crc32) of every byte before it (u32)
--tile (Codec(tile=(th, tw))): format 2.  The autoencoder still sees the whole image; the symbol volume is cut into tiles of th x tw
latent positions (all channels), each coded as a volume of its own -- own padding, own stream, first symbol uncoded -- so all tiles
decode concurrently (ic_pc_decode_tiles_f32, one work-group per tile) and damage stays inside a tile.  The price is the context lost
at tile borders and one stream termination per tile.  Without --tile every byte is format 1 as above; decompress reads both.
    0       4     magic  b'ICVF'
    4       2     format version (u16) = 2
    ..            ae name, pc name, H, W, C, h, w, L (u16), resolution (f64), fingerprint (u32): as version 1, without first_sym
    ..      2+2   th, tw (u16, u16): tile extent in symbol-volume units
    ..      4     ntiles (u32) = ceil(h / th) * ceil(w / tw)
    ..      6*nt  per tile, raster order: first_sym (u16), stream length in bytes (u32)
    ..      8     payload length n (u64) = the sum of the stream lengths
    ..      n     payload: the tiles' streams back to back, in table order
    ..      4     CRC-32 of every byte before it (u32)
--tile --checked (Codec(tile=(th, tw), checked=True)): format 4, "checked tiles" -- format 2 with a CRC-32 per tile stream and one
over the header, 4 * ntiles + 4 bytes more, the streams the same bytes.  decompress reads it with the strictness of format 2 (any
flipped bit, any truncation is refused).  salvage (Codec.salvage / salvage_many, --salvage) reads what a damaged format-4 file still
holds: after a header that passes its own CRC, every tile whose bytes are there and match their CRC is decoded, the others are
filled on the device from their intact neighbours (ic_pc_conceal_tiles) and named in the report.  verify checks files on the host.
    0       4     magic  b'ICVF'
    4       2     format version (u16) = 4        (3 is not used and is refused)
    ..            ae name, pc name, H, W, C, h, w, L, resolution, fingerprint, th, tw, ntiles: as version 2
    ..      10*nt per tile, raster order: first_sym (u16), stream length in bytes (u32), CRC-32 of that tile's stream bytes (u32)
    ..      8     payload length n (u64) = the sum of the stream lengths
    ..      4     header CRC-32: of every byte before it (magic up to and including the payload length)
    ..      n     payload: the tiles' streams back to back, in table order
    ..      4     CRC-32 of every byte before it (u32)
--tile --wavefront (Codec(tile=(th, tw), order='wavefront')): format 5, "wavefront tiles" -- the layout of format 4 byte for byte
(header, 10-byte tile rows with a CRC per stream, header CRC, file CRC; --checked is implied), version 5, but a tile's stream codes
its symbols in wavefront order: sorted by (T, c, y, x) with T = x + 2 y + 4 c in the tile's own coordinates (wavefront_order; every
tile by its own extent), the first of them -- (0, 0, 0) -- uncoded as first_sym.  The four masked layers of the context model make a
symbol depend only on symbols of smaller T (wavefront_is_valid derives that from the masks), so the decoder evaluates the network
for all symbols of one T at once and only the range decoder's step per symbol stays serial.  The tables are those of the tile coded
as its own volume, as in format 2; only their order in the stream differs.  salvage and verify read it like format 4.
Every failure of parse / decompress is a ValueError that names the cause; nothing of a refused file reaches the device.
The -dir commands and Codec.compress_many / decompress_many work on a list of images at once: the same bytes and the same pixels as
the single-image calls, file by file, but the tiles of all files are coded by one launch each way (ic_pc_decode_tiles_batch_f32: one
work-group per tile, whichever file it belongs to) and up to four autoencoder passes are in flight.  The file formats are unchanged.
--channels K (decompress*(channels=K)): a preview from the first K of the C latent channels of any file of any format.  Only those
are decoded; the others get fill_symbol(centres), the centre nearest zero, which is what the quantiser emits where the importance
map has masked a channel -- the decoder network knows such volumes (preview_symbols is the rule).  Raster streams (formats 1, 2, 4)
code (c, y, x) order, so the decoder stops after a prefix of every stream: (K + 3) / (C + 3) of its steps.  A format-5 decoder
must step through the symbols of later channels that share a front with wanted ones (wavefront_prefix_count) and saves less.
All CRCs are checked as always; damage in the bytes a preview does not reach cannot show in the decoder's status.
--tile --layers a,b,.. / --tile --progressive (Codec(tile=(th, tw), layers=[..] | 'default')): format 6, "layered tiles" -- a progressive
file.  Autoencoder, tiling and tables are those of formats 2 and 4 (every tile a volume of its own, raster order, first symbol
uncoded); only the cutting and the placing of the coded bytes differ.  Layer ends e_0 < e_1 < .. < e_{G-1} = C, 1 <= G <= 16: layer g
holds channels [e_{g-1}, e_g), e_{-1} = 0 (--progressive: default_layer_ends(C) = C/8, C/4, C/2, C).  Segment (t, g) is the range coder
started afresh over tile t's symbols of layer g in raster order, over those symbols' rows of the tile's own tables, terminated like
every stream: arithmetic_coding.encode_sequence(flat[a:b], freqs[a:b]) with a = max(1, e_{g-1} th' tw'), b = e_g th' tw'.  The context
crosses the layer boundaries (the lower channels are known to the decoder), only the coder state restarts; G = 1 is the format-4
stream of every tile.  The payload holds the segments LAYER first, so the bytes [0, layer_prefix_bytes(g)) are the header and the
layers 0 .. g - 1 of every tile: a reader holding them decodes channels 0 .. e_{g-1} - 1 of the whole image (decompress --partial,
Codec.decompress_partial; the other channels as in a --channels preview).
    0       4     magic  b'ICVF'
    4       2     format version (u16) = 6
    ..            ae name, pc name, H, W, C, h, w, L, resolution, fingerprint, th, tw, ntiles: as version 4
    ..      2     G, the number of layers (u16)
    ..      2*G   layer ends e_0 .. e_{G-1} (u16 each)
    ..      2*nt  first_sym per tile, raster order (u16)
    ..      8*G*nt segment table, LAYER-major (for g: for t:): length in bytes (u32), CRC-32 of the segment's bytes (u32)
    ..      8     payload length n (u64) = the sum of the lengths
    ..      4     header CRC-32: of every byte before it
    ..      n     payload: the segments in table order (all tiles' layer 0, then all tiles' layer 1, ..)
    ..      4     CRC-32 of every byte before it (u32)
decompress reads it as strictly as format 4; salvage of format 6 is not offered; verify checks it on the host.
--recover (Codec.recover / recover_many, parse_recover): what a damaged or cut format-6 file still holds, tile by tile.  Every segment
has its own length and CRC, so behind a header that passes its CRC every tile is read up to its own leading layers that are wholly
there and match their CRCs (an intact segment behind a damaged one cannot be decoded: the coder's context is missing): one flipped
bit costs one tile its upper layers, a download cut inside layer g keeps layer g of the tiles in front of the cut.  The decoder takes
a channel limit per tile (ic_pc_decode_tiles_batch_layers_pertile_f32); then every missing (tile, channel) is filled on the device
from the neighbouring tiles that hold that channel (ic_pc_conceal_tiles_channels: the most frequent symbol on the four edges, ties
to the smallest), or with the fill symbol where no neighbour holds it -- if all tiles stop at one layer, that is --partial's image.
The report names every tile with fewer than all layers.  --partial and --salvage read as before.
--tile --front-layers a,b,.. / --tile --front-progressive (Codec(tile=(th, tw), front_layers=[..] | 'default')): format 8, "front-layered
tiles" -- the bytes of format 6 (G, ends, first symbols, a length and a CRC per segment, header CRC, segments layer first, file CRC) with
version 8 (7 is not used and is refused); only the meaning of a segment differs, as format 5 reuses format 4's layout.  A tile's
symbols are coded in the wavefront order of format 5 and that stream is cut at FRONTS, not at channel planes (which are no prefix of
it): for a tile of extent (C, th', tw'), segment g holds the symbols of wavefront_order(C, th', tw') with index in [n_{g-1}, n_g),
n_g = wavefront_prefix_count(C, th', tw', e_g), n_{-1} = 0 (front_layer_cuts; index 0 is the uncoded first symbol; edge tiles have their
own cuts; e_0 = 1 on a 1 x 1 tile gives an empty segment, the one byte 0x80).  These are the symbols a --channels e_g decode of a
format-5 file steps through, so the bytes [0, layer_prefix_bytes(g)) decode as that preview a front at a time
(ic_pc_decode_tiles_batch_fronts_f32 restarts the coder at each cut).  The price: a layer's prefix also carries the symbols of later
channels that share its fronts, so the early prefixes are longer than format 6's; nothing is coded twice.  decompress, --channels,
--partial, --recover and verify read it as they read format 6, and so does stream --fronts; --salvage and stream without it do not.
--tile --depth [--depth-block B] (Codec(tile=(th, tw), depth_block=B)): format 10, "depth-mapped tiles" -- the layout of formats 4 / 5
(a CRC per tile and one over the header, always) with the depth block B (default 4, 1 .. 255) as one '<H' behind the tile extent; 9
is not used and is refused.  Every tile's stream is a DEPTH PLANE followed by the range coder's bytes, and the tile's CRC covers both.
The plane (depth_plane) has one byte per block of B x B latent cells, counted from the tile's corner, ragged at the far edges: 0 if
every symbol of the block's cells is the fill symbol (fill_symbol: the centre nearest zero, what the importance map and a --cap leave
in the channels they mask), else 1 + the largest channel that holds another symbol in any of them.  Position (c, y, x) of a tile is
LIVE iff c < depth[y // B][x // B]; the coder's bytes are those of format 5 over the live positions alone (depth_live_mask: the
wavefront order with the dead positions left out; index 0 is still the uncoded first symbol), and a dead position decodes to the fill
symbol without a coder step -- the depth wins over the first symbol.  So neither side pays for a symbol that carries nothing, a capped
or region-of-interest file decodes as fast as its content allows without --channels, and a tile whose upper channels are dead
everywhere ends its front sweep early.  The plane is stored raw: 16 bytes per 16 x 16 tile at B = 4, 64 at B = 2, 256 at B = 1.
parse_container refuses, naming the tile, a stream shorter than its plane and a depth above C; C > 255 is refused for this format.
decompress, --channels K, --region, the -dir commands, transcode to and from it, measure, rd and the searches read and write it like
format 5; verify and info are host only (info prints B, the live share and the front steps per tile the depths imply).  --salvage,
--partial, --recover, stream and repair refuse a format-10 file in one sentence.  Not with --wavefront or the layered formats; a
context model the wavefront order refuses, or of another width than k = 24, is refused.
--tile --rans [--lanes W] (Codec(tile=(th, tw), rans=W | 'default')): format 12, "lane-parallel rANS tiles" -- the layout of format 10
with the number of coders W (8, 16, 32 or 64, default 16) as the '<H' where format 10 keeps its block size; 11 is not used and is
refused.  Every tile's stream is that of W interleaved rANS coders: position (c, y, x) lies on front t = x + 2 y + 4 c, where it has
the candidate index e of the front decoder's enumeration (rans_slot); coder e mod W codes it in round (t, e div W) (rans_rounds), so
the decoder steps W coders at once where format 5 steps one.  The coder's table is an integer function of the arithmetic coder's
(rans_table: M = 2^16, g_j = max(1, f_j (M - L) // sum f), the deficit to the first largest f_j); the stream is the W final states,
then the 16-bit words in the order the decoder takes them (rans_encode / rans_decode are the host statement, tests/rans_rule.py the
slow one).  A full decode checks that every coder rests at 2^16 and that the words end the stream.  decompress, --channels K,
--region, the -dir commands, transcode to and from it, measure, rd and the searches read and write it like format 5; verify and info
are host only (info prints W and the states' share of the payload).  --salvage, --partial, --recover, stream and repair refuse a
format-12 file in one sentence.  Not with --checked, --wavefront, --depth or the layered formats; a context model the wavefront order
refuses, or of another width than k = 24, is refused.
stream (Codec.open_stream -> StreamDecoder): a format-6 file that is still arriving.  feed(chunk) takes the bytes as they come, image()
gives recover's picture and report of the bytes so far -- but the decoder goes on where the last image() stopped: the session
(PredictionNetwork.open_layers) keeps every tile's decoder workspace on the device and ic_pc_decode_tiles_batch_layers_resume_f32
continues each tile at the first layer it has gained (resume_plan), so a viewer that redraws after every layer decodes every channel
plane once, not once per redraw.  The command feeds IN.icf in chunks of --chunk bytes (default 16384), as a download would, and
writes OUT_DIR/<stem>.<bytes fed, 9 digits>.png with a recover line each time a tile has gained a layer; the last picture of an intact
file is decompress's.
stream --fronts (Codec.open_stream(fronts=True)): a format-8 file is streamed too.  The session is opened with the file's ends as front
ends and ic_pc_decode_tiles_batch_fronts_resume_f32 continues every tile's front sweep behind the last front of the layers it held, so
every front is swept once: the 191 steps of a (32, 16, 16) tile in all, where a --recover per redraw at the four default layer ends
takes 79 + 95 + 127 + 191.  Opt-in: without --fronts a format-8 file is refused as before.  A format-6 file streams the same either way.
--cap / --roi / --background / --max-bytes / --bpp (Codec.compress(cap=, rois=, background=), compress_to_budget): the encoder's rate
knob.  The importance map heatmap2D = sigmoid(z0) C says per latent position how many of the C channels carry information; a cap is
an upper bound on it, one float per position (cap_plane): the same level everywhere is a rate below the trained point, a plane that
is high inside rectangles and low outside is region-of-interest coding, a search over the level (cap_levels: the grid k C / 256;
budget_search: the contract, established on real files) is a byte budget.  A capped channel quantises to the centre nearest zero,
the value every decoder path already knows as "nothing here" (fill_symbol), so the file format does not change, the cap is not
recorded in the file and reading needs no option.  The budget search runs the encoder once and requantises its bottleneck per
level (ic_heatmap_quantize_cap_f32: up to 16 levels a launch, costed by the context model as one batch for the estimate).
transcode / transcode-dir (Codec.transcode, transcode_many, transcode_to_budget, repair): a file to a file, without its image.  A file
is a symbol volume plus a choice of entropy-coding layout; the symbols are the autoencoder's, so they are decoded, left on the device
and coded again in the format this Codec writes -- byte for byte the file compress would have written from the image, where
compress(decompress(data)) runs the autoencoder twice and yields other symbols.  No new format, no new entry point: the decoders and
encoders above, and between them at most one torch.where.  An INTEGER cap K gives exactly preview_symbols(plain, K, fill) (the
quantiser's contract), so --cap / --roi / --background at integer levels and --max-bytes / --bpp over the levels 0 .. C
(budget_search(steps=C)) apply to a file as they apply to an image: cap_symbols is the rule, cell p keeps the channels below its
level.  A fractional level rescales z and needs the bottleneck: refused here, it is compress's.  --salvage / --recover (repair) write
what a damaged format-4 / 5 (salvage's reader and concealment) or a damaged or cut format-6 / 8 file (recover's) still holds as an
intact file, with the reader's report; formats 1 and 2 carry no checksums to read a damaged file by.
decompress --region (Codec.decompress_region, decompress_regions_many, region_plan, decoder_reach): a pixel rectangle of a tiled file
from the tiles it needs.  A pixel depends on a bounded block of latent cells (decoder_reach walks the decoder's layers: 4 n3 + 3
pixels before a cell's 8 x 8 block and 4 n3 + 10 behind it, n3 = 6 B + 2; 18 and 17 cells for B = 5), so the rectangle names a
range of tile rows and columns (region_plan); their streams are decoded as a volume of their own and the autoencoder's decoder runs
over that window with the kernel forms of the whole picture forced on it (Autoencoder.plan_like), which keeps the pixels those of
decompress bit for bit; where the picture runs F(4x4) kernels the window is wider (decoder_cells: the transforms carry rounding in
from about twice as far), and where the forms cannot be had on the window the whole picture is decoded and cropped.  The whole file is
parsed and checked whatever the rectangle.  No new format, entry point or kernel: the launches above over fewer tiles and a smaller
map.  info prints region_plan for a file on the host.
measure / rd / --min-psnr / --min-ms-ssim (Codec.measure, rd_curve, compress_to_quality, transcode_to_quality; quality_search): the other
axis of the rate knobs.  measure decodes a file, leaves the picture on the device and puts it and the uploaded original through
metrics.val_metrics_device (float64, the operations of the NumPy code val.py reports) -> Measure(bytes, bpp, mse, psnr, ms_ssim), of the
whole picture or of a rectangle.  rd_curve runs the encoder once, requantises its bottleneck 16 levels a launch, codes every level to a
real file and decodes every level by a batch-1 pass of its own (the kernel form of a layer depends on the batch size; the pixels must be
decompress's), so row i is measure(img, compress(img, cap=level_i)) in every field.  compress_to_quality searches cap_levels for the
smallest level whose picture reaches a PSNR or an MS-SSIM; a probe is a requantisation, a decode and a metrics call, nothing is
entropy-coded until the level is found.  Quality need not be monotone in the level (under untrained weights it is not), so
quality_search -- budget_search on the mirrored index -- establishes both halves of its contract by calls: the level meets the target,
the next one down does not.  transcode_to_quality does the same for a file over the integer levels 0 .. C against the picture the file
decodes to now, without the encoder.  No new kernel, entry point or format.  With synthetic weights the numbers mean nothing.
--rdo LAMBDA (Codec.compress(rdo=), compress_many(rdos=), choose_symbols, rdo_curve; ilog2_q16, rdo_choose, rdo_record): rate-aware symbol
choice at encode.  The knobs above cut channels; this one asks the context model what a symbol costs.  After the encoder pass every
tile of the Codec's grid (the whole volume for format 1) is swept front by front -- the sweep of the wavefront decoder, on the device:
PredictionNetwork.choose_tiles_batch, IC_PC_DECODE_RDO -- and every position takes the first symbol that attains the minimum of
float64(k_j) + Lambda * float64(R_j): k_j the hard quantiser's own float32 key of centre j, R_j = ilog2_q16(T) - ilog2_q16(f_j) the rate
in 2^-16 bits over the coder's own integer table of the position given the symbols already chosen, Lambda = lambda 1e7 / 65536.  A chosen
symbol is final (the greedy rule).  rdo_choose states the rule of one position on the host; the device equals it exactly.  lambda = 0 is
the quantiser, and the file of compress byte for byte.  The symbols are coded in whatever format the Codec writes and read by every
reader as ever: no new format, no new entry point.  A search over lambda for a budget or a quality is not offered.
"""
import argparse
import io
import json
import os
import re
import struct
import sys
import zlib
from collections import namedtuple

import numpy as np

MAGIC = b'ICVF'
FORMAT_VERSION = 1
_MIN_SIZE = 4 + 2 + 2 + 2 + 8 + 10 + 2 + 2 + 8 + 4 + 8 + 4        # both names empty, no payload

Container = namedtuple('Container', ['version', 'ae_name', 'pc_name', 'H', 'W', 'C', 'h', 'w', 'L', 'first_sym',
                                     'resolution', 'fingerprint', 'payload'])


FORMAT_VERSION_TILED = 2
TiledContainer = namedtuple('TiledContainer', ['version', 'ae_name', 'pc_name', 'H', 'W', 'C', 'h', 'w', 'L', 'resolution', 'fingerprint',
                                               'th', 'tw', 'first_syms', 'streams', 'payload'])


FORMAT_VERSION_CHECKED = 4                                           # 3 is not used: it stays "unsupported"
CheckedContainer = namedtuple('CheckedContainer', TiledContainer._fields + ('stream_crcs',))
FORMAT_VERSION_WAVEFRONT = 5                                         # the layout of 4, the streams in wavefront order
WavefrontContainer = namedtuple('WavefrontContainer', CheckedContainer._fields)
FORMAT_VERSION_LAYERED = 6                                           # raster tiles cut into layers, stored layer first
FORMAT_VERSION_FRONTS = 8                                            # wavefront tiles cut into layers at fronts; 7 is not used
_LAYERED_VERSIONS = (FORMAT_VERSION_LAYERED, FORMAT_VERSION_FRONTS)  # one layout, one container type: `version` tells them apart
MAX_LAYERS = 16
# streams[t] is tile t's list of G segments (what decode_tiles_batch(layer_ends=...) takes), segments[g][t] the same bytes layer-major
# (the file's order), segment_crcs[g][t] their CRCs; a segment that parse_partial found incomplete is None in both views.  version is
# 6 (segments cut at channel planes of the raster order) or 8 (cut at fronts of the wavefront order, front_layer_cuts)
LayeredContainer = namedtuple('LayeredContainer', TiledContainer._fields + ('layer_ends', 'segments', 'segment_crcs'))
PartialReport = namedtuple('PartialReport', ['layers_total', 'layers_decoded', 'channels', 'file_crc_ok'])
FORMAT_VERSION_DEPTH = 10                                            # format 5 plus a depth plane per tile; 9 is not used
DEFAULT_DEPTH_BLOCK = 4
# streams[t] is tile t's depth plane (ceil(th' / B) * ceil(tw' / B) bytes, row-major, blocks counted from the tile's corner) followed
# by the range coder's bytes over the tile's live positions; depth_block is B
DepthContainer = namedtuple('DepthContainer', CheckedContainer._fields + ('depth_block',))
FORMAT_VERSION_RANS = 12                                             # wavefront tiles coded by W interleaved rANS coders; 11 is not used
RANS_LANES = (8, 16, 32, 64)
DEFAULT_RANS_LANES = 16
RANS_M = 1 << 16                                                     # the coder's table total and word size: fixed by format 12
# streams[t] is tile t's W final coder states ('<I' each, lane l at byte 4 l) followed by the 16-bit words in the order the decoder
# takes them; lanes is W
RansContainer = namedtuple('RansContainer', CheckedContainer._fields + ('lanes',))
# One row per format version: what the builders, the readers and Codec look up where they would branch on the version.
#   container    the namedtuple parse_container gives; name: what messages call the format
#   checked      a CRC per stream or segment in the tile table and one over the header
#   extra        the one '<H' behind the tile extent, by the name of its container field; check_extra(value, C) validates it
#   layered      segments per tile, stored layer first (the layout of format 6)
#   order        what encode_tiles* and decode_tiles_batch are told as order= (None: not told)
#   param_kw     the keyword that carries the format's parameter to them: the layer ends or the extra field
#   refusals     the Codec attributes that hold the model's refusal of the format, in the order a reader asks them
#   readers      which readers of damaged or cut files take it: 'salvage' (--salvage) or 'partial' (--partial, --recover, stream); repair
#                takes what either takes
Format = namedtuple('Format', ['version', 'container', 'name', 'checked', 'extra', 'check_extra', 'layered', 'order', 'param_kw',
                               'refusals', 'readers'])
FORMATS = {row.version: row for row in (
    Format(FORMAT_VERSION, Container, 'one stream', False, None, None, False, None, None, (), ()),
    Format(FORMAT_VERSION_TILED, TiledContainer, 'tiles', False, None, None, False, 'raster', None, (), ()),
    Format(FORMAT_VERSION_CHECKED, CheckedContainer, 'checked tiles', True, None, None, False, 'raster', None, (), ('salvage',)),
    Format(FORMAT_VERSION_WAVEFRONT, WavefrontContainer, 'wavefront tiles', True, None, None, False, 'wavefront', None,
           ('wavefront_refusal',), ('salvage',)),
    Format(FORMAT_VERSION_LAYERED, LayeredContainer, 'layered tiles', True, None, None, True, None, 'layer_ends',
           ('layered_refusal',), ('partial',)),
    Format(FORMAT_VERSION_FRONTS, LayeredContainer, 'front-layered tiles', True, None, None, True, None, 'front_ends',
           ('layered_refusal', 'wavefront_refusal'), ('partial',)),
    Format(FORMAT_VERSION_DEPTH, DepthContainer, 'depth-mapped tiles', True, 'depth_block', lambda B, C: check_depth_block(B, C), False,
           'wavefront', 'depth_block', ('depth_refusal',), ()),
    Format(FORMAT_VERSION_RANS, RansContainer, 'lane-parallel rANS tiles', True, 'lanes', lambda W, C: check_rans_lanes(W), False,
           'rans', 'lanes', ('rans_refusal',), ()))}
_TILED = tuple(dict.fromkeys(row.container for row in FORMATS.values() if row.container is not Container))
_WITH_CRCS = tuple(v for v, row in FORMATS.items() if 'salvage' in row.readers)      # the formats salvage reads
WAVEFRONT_COEFFS = (2, 4)                                            # T = x + 2 y + 4 c: fixed by format 5

# what salvage tells about a file: damaged is [DamagedTile] in tile order; latent = (y0, x0, th, tw) in the symbol volume, pixels =
# (y0, x0, height, width) in the returned image, clipped to it (height or width 0: the tile lies in the padding)
DamagedTile = namedtuple('DamagedTile', ['index', 'reason', 'latent', 'pixels'])
SalvageReport = namedtuple('SalvageReport', ['ntiles', 'file_crc_ok', 'damaged'])
# what recover tells about a layered file: tiles is [RecoveredTile] in tile order, only the tiles with fewer than all layers; layers /
# channels = what was decoded of the tile, reason = 'crc' | 'truncated' (the first segment that could not be read) | 'decoder';
# latent and pixels as in DamagedTile
RecoveredTile = namedtuple('RecoveredTile', ['index', 'layers', 'channels', 'reason', 'latent', 'pixels'])
RecoverReport = namedtuple('RecoverReport', ['ntiles', 'layers_total', 'file_crc_ok', 'tiles'])


def tile_grid(h, w, th, tw):
    """the tiles of an (h, w) latent plane cut into th x tw blocks: [(y0, x0, th', tw')] in raster order, ceil(h / th) * ceil(w / tw)
    of them, the last row / column smaller where th / tw does not divide; every position is in exactly one tile."""
    h, w, th, tw = int(h), int(w), int(th), int(tw)
    if h < 1 or w < 1 or th < 1 or tw < 1:
        raise ValueError('tile grid: plane {} x {} and tile {} x {} must all be at least 1'.format(h, w, th, tw))
    return [(y0, x0, min(th, h - y0), min(tw, w - x0)) for y0 in range(0, h, th) for x0 in range(0, w, tw)]


CAP_STEPS = 256                                                      # cap_levels: the grid a budget is searched on


def cap_levels(C):
    """the CAP_STEPS + 1 levels fl32(k C / CAP_STEPS), k = 0 .. CAP_STEPS, of an importance-map cap: 0 (every channel masked) up
    to C (no cap); for C = 32 the step is 0.125"""
    return (np.arange(CAP_STEPS + 1, dtype=np.float64) * int(C) / CAP_STEPS).astype(np.float32)


def _check_level(value, what):
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError('{} {!r} is not a number'.format(what, value))
    if not v >= 0.0:                                                 # (a NaN compares false)
        raise ValueError('{} {} is not in [0, +inf]'.format(what, value))
    return v


def cap_plane(H, W, factor, level=None, rois=(), background=None):
    """the (h, w) float32 cap of an H x W image for Codec.compress(cap=...): `level` (None: +inf, no cap) in every latent cell, or,
    with rectangles rois = [(x, y, w, h), ..] in pixels of the image, `level` in the cells whose factor x factor block of the
    padded image (val.add_padding pads centred: top ((-H) % factor) // 2, left likewise) intersects a rectangle and `background` in
    the others.  A ValueError for a level outside [0, +inf], a rectangle of no extent or one that misses the image, rectangles
    without a background."""
    H, W, f = int(H), int(W), int(factor)
    if H < 1 or W < 1 or f < 1:
        raise ValueError('cap_plane: image {} x {}, factor {}'.format(H, W, f))
    h, w = (H + f - 1) // f, (W + f - 1) // f
    inside = np.float32(np.inf if level is None else _check_level(level, 'level'))
    rois = list(rois) if rois is not None else []
    if not rois:
        if background is not None:
            raise ValueError('background {} without a rectangle: the level alone is the cap of every cell'.format(background))
        return np.full((h, w), inside, dtype=np.float32)
    if background is None:
        raise ValueError('a region of interest needs a background: the level of the cells outside the rectangles')
    plane = np.full((h, w), np.float32(_check_level(background, 'background')), dtype=np.float32)
    top, left = ((-H) % f) // 2, ((-W) % f) // 2
    for r in rois:
        x0, y0, x1, y1 = _clip_rect(r, H, W)
        plane[(y0 + top) // f:(y1 - 1 + top) // f + 1, (x0 + left) // f:(x1 - 1 + left) // f + 1] = inside
    return plane


def _clip_rect(rect, H, W):
    """(x, y, w, h) in pixels of an H x W image -> (x0, y0, x1, y1) clipped to it; the ValueErrors of cap_plane's rectangles"""
    try:
        x, y, rw, rh = (int(v) for v in rect)
    except (TypeError, ValueError):
        raise ValueError('rectangle {!r} is not (x, y, w, h) in pixels'.format(rect))
    if rw < 1 or rh < 1:
        raise ValueError('rectangle {}: the extent {} x {} is not positive'.format((x, y, rw, rh), rw, rh))
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + rw, W), min(y + rh, H)
    if x0 >= x1 or y0 >= y1:
        raise ValueError('rectangle {} does not intersect the {} x {} image'.format((x, y, rw, rh), W, H))
    return x0, y0, x1, y1


def decoder_layers(B):
    """the decoder network as a list of (kernel extent, upsampling): what weights.ae_conv_specs names below autoencoder/decoder --
    from_bn (3 x 3 transposed, stride 2), 6 B + 2 convolutions of 3 x 3, h12 and h13 (5 x 5 transposed, stride 2)"""
    from .weights import ae_conv_specs, DEC
    B = int(B)
    if B < 0:
        raise ValueError('decoder layers: B = {} is negative'.format(B))
    return [(int(shape[0]), 2 if kind == 'deconv' else 1) for scope, kind, shape in ae_conv_specs(1, B) if scope.startswith(DEC + '/')]


def _f4_needs(a, b):
    """the positions whose VALUES the F(4x4, 3x3) kernels read for the outputs a .. b of a 3 x 3 convolution, tiles of 4 from position
    0: in exact arithmetic an output needs its 3 neighbours, but the transforms mix a tile's 6 inputs -- y0 = m0 + .. + m4 of
    t0 .. t4 takes d0 .. d4 (positions 4 t - 1 .. 4 t + 3), y1 and y2 take d1 .. d4, y3 = .. + m5 takes d1 .. d5 (w4_bt / w4_at of
    conv3x3_wino4.hip) -- and what cancels in exact arithmetic leaves its rounding.  F(2x2) has no such term: its y0 takes d0 .. d2."""
    return 4 * (a // 4) - (1 if a % 4 == 0 else 0), 4 * (b // 4) + (4 if b % 4 == 3 else 3)


def decoder_cells(p0, p1, B, f4_convs=False, f4_h12=False):
    """the latent cells whose values the decoder's kernels read for the pixels p0 .. p1 (inclusive) of the padded picture, along
    one axis -> (first, last), not clipped to the plane.  Walked backwards through decoder_layers.  With both flags False it is the
    dependency in exact arithmetic, ceil((p0 - 7 - after) / 8) .. floor((p1 + before) / 8) of decoder_reach -- which is also what
    the direct and the F(2x2) kernels read.  f4_convs: the 3 x 3 layers run F(4x4) (_f4_needs: about two positions a layer instead
    of one).  f4_h12: h12 runs as F(4x4) 3 x 3 convolutions over the four phases of its output, position i of H/2 in tile i // 2 of H/4.
    A window that holds these cells gives the picture's values bit for bit under the picture's kernels, not only close ones."""
    a, b = int(p0), int(p1)
    layers = decoder_layers(B)
    for n in range(len(layers) - 1, -1, -1):
        k, up = layers[n]
        if up == 2 and f4_h12 and n == len(layers) - 2:
            a, b = _f4_needs(a // 2, b // 2)
        elif up == 2:
            pad = (k - 2) // 2                                       # output o takes input i with o = 2 i + t - pad, t = 0 .. k - 1
            a, b = -((k - 1 - pad - a) // 2), (b + pad) // 2
        elif f4_convs and k == 3:
            a, b = _f4_needs(a, b)
        else:
            a, b = a - k // 2, b + k // 2
    return a, b


def decoder_reach(B):
    """how far a latent cell reaches in the decoded picture -> (before, after) in pixels: a change of cell c changes pixels of
    [f c - before, f c + f - 1 + after] at most, f = 8 the subsampling factor; 4 n3 + 3 and 4 n3 + 10 with n3 = 6 B + 2.  Walked
    through decoder_layers: a SAME convolution of extent k widens an interval [a, b] to [a - k // 2, b + k // 2]; a stride-2
    transposed one -- the adjoint of the SAME convolution 2 n -> n, whose pad in front is (k - 2) // 2 -- maps it to
    [2 a - (k - 2) // 2, 2 b + k - 1 - (k - 2) // 2].  Equivalently pixel p of the padded picture depends on the cells c with
    ceil((p - (f - 1) - after) / f) <= c <= floor((p + before) / f)."""
    a, b, f = 0, 0, 1
    for k, up in decoder_layers(B):
        if up == 1:
            a, b = a - k // 2, b + k // 2
        else:
            pad = (k - 2) // 2
            a, b, f = 2 * a - pad, 2 * b + k - 1 - pad, 2 * f
    return -a, b - (f - 1)


RegionPlan = namedtuple('RegionPlan', ['rect', 'rows', 'cols', 'tiles', 'window', 'offset'])


def region_plan(H, W, factor, h, w, th, tw, rect, reach, align=1):
    """which tiles a pixel rectangle of an H x W image needs, on the host.  rect = (x, y, w, h) in pixels of the image, clipped to
    it (a ValueError for a rectangle of no extent or one that misses the image, as cap_plane's); the image sits in the padded
    picture at val.add_padding's centred offsets (top ((-H) % factor) // 2, left likewise); reach = (before, after) of
    decoder_reach -- or a function (p0, p1) -> (first cell, last cell) for the padded pixels p0 .. p1 of one axis, as decoder_cells
    is, where the kernels read more than the arithmetic needs; (h, w) the latent plane, cut by tile_grid(h, w, th, tw).  -> RegionPlan:
        rect    (x, y, w, h), clipped
        rows    (r0, r1), cols (c0, c1): the tile rows r0 .. r1 - 1 and tile columns c0 .. c1 - 1 that hold a cell a pixel of the
                rectangle depends on -- pixel p depends on the cells ceil((p - (factor - 1) - after) / factor) .. floor((p + before) /
                factor), clipped to the plane
        tiles   their indices in tile_grid(h, w, th, tw), raster order
        window  (y0, x0, wh, ww) in cells, the block those tiles cover: y0 = r0 th, wh = min(h, r1 th) - y0 and likewise across --
                cut at the tile grid, never inside a tile, so tile_grid(wh, ww, th, tw) is exactly those tiles, a ragged last row
                or column included
        offset  (oy, ox): the rectangle's corner inside the window's decoded picture, in pixels
    align = A > 1: r0 and c0 go down to the next tile whose first cell is a multiple of A (the window may then hold a row or a
    column of tiles the rule does not ask for): the decoder's F(4x4) kernels cut the plane at H/4 into 4 x 4 tiles from the corner,
    2 x 2 cells, and a window's tiles must fall where the picture's do."""
    H, W, f, h, w, th, tw, A = int(H), int(W), int(factor), int(h), int(w), int(th), int(tw), int(align)
    if H < 1 or W < 1 or f < 1 or A < 1:
        raise ValueError('region_plan: image {} x {}, factor {}, align {}'.format(H, W, f, A))
    if (h, w) != ((H + f - 1) // f, (W + f - 1) // f):
        raise ValueError('region_plan: a {} x {} plane does not belong to a {} x {} image at factor {}'.format(h, w, H, W, f))
    tile_grid(h, w, th, tw)                                          # (its ValueError for an empty plane or tile)
    if callable(reach):
        cells = reach
    else:
        before, after = (int(v) for v in reach)
        cells = lambda p0, p1: (-((after + f - 1 - p0) // f), (p1 + before) // f)      # ceil((p0 - (f - 1) - after) / f), floor((p1 + before) / f)
    x0, y0, x1, y1 = _clip_rect(rect, H, W)
    top, left = ((-H) % f) // 2, ((-W) % f) // 2

    def tiles_of(p0, p1, n, t):                                      # padded pixels p0 .. p1 - 1 -> tile indices [t0, t1) of n cells cut by t
        lo, hi = cells(p0, p1 - 1)
        lo, hi = max(0, int(lo)), min(n - 1, int(hi))
        t0 = lo // t
        while (t0 * t) % A:
            t0 -= 1
        return t0, hi // t + 1

    r0, r1 = tiles_of(y0 + top, y1 + top, h, th)
    c0, c1 = tiles_of(x0 + left, x1 + left, w, tw)
    ncols = (w + tw - 1) // tw
    wy, wx = r0 * th, c0 * tw
    return RegionPlan((x0, y0, x1 - x0, y1 - y0), (r0, r1), (c0, c1), [r * ncols + c for r in range(r0, r1) for c in range(c0, c1)],
                      (wy, wx, min(h, r1 * th) - wy, min(w, c1 * tw) - wx), (y0 + top - wy * f, x0 + left - wx * f))


def budget_search(fits, estimate_index, steps=CAP_STEPS):
    """the largest-level search behind a byte budget, over the indices 0 .. CAP_STEPS of cap_levels.  fits(k) -> bool is one real
    coding at level k; estimate_index is advice.  -> (k, probes) with fits(k) true and k == CAP_STEPS or fits(k + 1) false, BOTH
    established by calls of fits: sizes need not be monotone in the level (tile borders, the context model), so the bisection
    keeps fits(lo) and not fits(hi) and ends on an adjacent pair whatever lies between.  Order: CAP_STEPS (returned if it fits);
    the estimate and, if it fits, its successor; 0 if no fitting index is known yet; then bisection of the side that remains --
    at most 1 + 2 + 1 + 8 calls, none repeated.  A ValueError if 0 does not fit.
    steps=S >= 1: the same search over the indices 0 .. S (Codec.transcode_to_budget: the integer levels 0 .. C), at most
    1 + 2 + 1 + ceil(log2 S) calls."""
    steps = int(steps)
    if steps < 1:
        raise ValueError('budget search: {} steps, at least 1 is needed'.format(steps))
    probes = [0]

    def probe(k):
        probes[0] += 1
        return bool(fits(k))

    hi = steps
    if probe(hi):
        return hi, probes[0]
    lo = None
    e = min(max(int(estimate_index), 0), steps - 1)
    if probe(e):
        lo = e
        if e + 1 < hi:
            if probe(e + 1):
                lo = e + 1
            else:
                hi = e + 1
    else:
        hi = e
    if lo is None:
        if hi == 0 or not probe(0):
            raise ValueError('no level fits: the smallest file, at level 0, is over the budget in bytes')
        lo = 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if probe(mid):
            lo = mid
        else:
            hi = mid
    return lo, probes[0]


def quality_search(meets, steps=CAP_STEPS):
    """the smallest-level search behind a quality target, over the indices 0 .. steps: budget_search run on the mirrored index.
    meets(k) -> bool is one decoded and measured picture at level k.  -> (k, probes) with meets(k) true and k == 0 or meets(k - 1)
    false, BOTH established by calls of meets: quality need not be monotone in the level (under untrained weights it is not), so the
    bisection keeps not meets(lo) and meets(hi) and ends on an adjacent pair whatever lies between.  Order: 0 (returned if it
    meets); steps and, if it meets, steps - 1; then bisection of what remains -- at most 1 + 2 + ceil(log2 steps) calls, none
    repeated (budget_search's 1 + 2 + 1 + ceil(log2 steps) with the estimate at the top, which saves its fourth call).  A ValueError
    if meets(steps) is false: the file without a cap misses the target."""
    steps = int(steps)
    if steps < 1:
        raise ValueError('quality search: {} steps, at least 1 is needed'.format(steps))
    seen = {}

    def fits(j):
        seen[steps - j] = bool(meets(steps - j))
        return seen[steps - j]

    try:
        j, probes = budget_search(fits, 0, steps=steps)
    except ValueError:
        if seen.get(steps) is not False:                             # (the error is meets's own)
            raise
        raise ValueError('no level meets the target: the top level, {}, does not'.format(steps))
    return steps - j, probes


Measure = namedtuple('Measure', ['bytes', 'bpp', 'mse', 'psnr', 'ms_ssim'])
MIN_MEASURE_SIDE = 16                                                # 2^4: one whole pixel at the last of MS-SSIM's five scales


def measure_from_values(values, nbytes, pixels):
    """the six float64 values of metrics.val_metrics_device (the five scale terms of MS-SSIM, then the mean squared error) and a
    file of nbytes bytes for `pixels` pixels -> Measure.  psnr = metrics.psnr_from_mse(mse); ms_ssim = metrics.msssim_from_scale_values,
    but nan where a scale term is negative (or nan), as the NumPy code's fractional power gives it -- the Python-float helper would
    return a complex number there."""
    from . import metrics
    vals = [float(v) for v in values]
    if len(vals) != 6:
        raise ValueError('measure: expected the 5 scale values and the mean squared error, got {} values'.format(len(vals)))
    scales, mse = vals[:5], vals[5]
    ms_ssim = metrics.msssim_from_scale_values(scales) if all(v >= 0 for v in scales) else float('nan')     # (a NaN compares false)
    return Measure(int(nbytes), 8.0 * int(nbytes) / int(pixels), mse, metrics.psnr_from_mse(mse), ms_ssim)


def check_measured_image(img_hwc_uint8, H, W):
    """the original handed to Codec.measure for a file of an H x W picture -> the (H, W, 3) uint8 array; a ValueError naming both
    shapes if it is not that picture's"""
    img = np.asarray(img_hwc_uint8)
    if img.ndim != 3 or img.shape[2] not in (3, 4) or img.dtype != np.uint8:
        raise ValueError('expected an HWC uint8 image with 3 channels, got {} {}'.format(img.shape, img.dtype))
    if img.shape[:2] != (int(H), int(W)):
        raise ValueError('the image is {} x {}, the file decodes to {} x {}: a measure compares a picture with its own original'.format(
            img.shape[0], img.shape[1], int(H), int(W)))
    return img[:, :, :3]


def measure_rect(rect, H, W):
    """the rect argument of Codec.measure -> (x0, y0, x1, y1) clipped to the H x W picture as a region of interest is (_clip_rect); a
    ValueError if less than MIN_MEASURE_SIDE pixels a side remain"""
    x0, y0, x1, y1 = _clip_rect(rect, H, W)
    if x1 - x0 < MIN_MEASURE_SIDE or y1 - y0 < MIN_MEASURE_SIDE:
        raise ValueError('rectangle {}: {} x {} pixels of it lie in the image, MS-SSIM needs at least {} a side'.format(
            tuple(int(v) for v in rect), x1 - x0, y1 - y0, MIN_MEASURE_SIDE))
    return x0, y0, x1, y1


def quality_target(psnr=None, ms_ssim=None):
    """exactly one of psnr (dB; +inf is a target, NaN is not) and ms_ssim (0 .. 1) -> (the Measure field, the value)"""
    if (psnr is None) == (ms_ssim is None):
        raise ValueError('a quality target is exactly one of psnr (dB) and ms_ssim (0 .. 1), got {}'.format(
            'both' if psnr is not None else 'neither'))
    name, value = ('psnr', psnr) if psnr is not None else ('ms_ssim', ms_ssim)
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError('{} target {!r} is not a number'.format(name, value))
    if v != v or (name == 'ms_ssim' and not 0.0 <= v <= 1.0):
        raise ValueError('{} target {} is not {}'.format(name, value, 'a number of dB' if name == 'psnr' else 'in 0 .. 1'))
    return name, v


def meets_target(measure, name, value):
    """does a Measure reach the target of quality_target?  A nan never does."""
    return bool(getattr(measure, name) >= value)


def rd_levels(C, n=16):
    """the n + 1 levels k C / n, k = 0 .. n, of a rate-distortion table (--levels N), 1 <= n <= CAP_STEPS -> list of float"""
    if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= CAP_STEPS:
        raise ValueError('--levels {!r}: the table has N + 1 levels k C / N with N an integer in 1 .. {}'.format(n, CAP_STEPS))
    return [float(k) * int(C) / int(n) for k in range(int(n) + 1)]


def check_rd_levels(levels, C):
    """the levels argument of Codec.rd_curve: None (rd_levels(C)) or a non-empty increasing sequence of levels in [0, +inf]"""
    if levels is None:
        return rd_levels(C)
    try:
        out = [_check_level(v, 'level') for v in levels]
    except TypeError:
        raise ValueError('levels {!r} are not a sequence of numbers'.format(levels))
    if not out or any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError('levels {} are not a non-empty increasing sequence'.format(out))
    return out


def wavefront_dependencies(masks, num_layers):
    """the positions a symbol's table depends on, as offsets (dc, dy, dx) from it: masks = (first mask, other mask), each
    (KD, KH, KW[, 1, 1]) with the current position at the centre of the last slice; the first layer uses the first mask, the
    num_layers - 1 layers behind it the other one.  The set is the Minkowski sum of the layers' live offsets."""
    first, other = (np.asarray(m, dtype=np.float64) for m in masks)
    first, other = first.reshape(first.shape[:3]), other.reshape(other.shape[:3])
    if int(num_layers) < 1:
        raise ValueError('a context model has at least one layer, got {}'.format(num_layers))

    def live(mask):
        KD, KH, KW = mask.shape
        return [(kd - (KD - 1), kh - KH // 2, kw - KW // 2) for kd in range(KD) for kh in range(KH) for kw in range(KW) if mask[kd, kh, kw] != 0]

    deps = set(live(first))
    for _ in range(int(num_layers) - 1):
        step = live(other)
        deps = set((a[0] + b[0], a[1] + b[1], a[2] + b[2]) for a in deps for b in step)
    return deps


def wavefront_is_valid(masks, num_layers, a, b):
    """does T = x + a y + b c order the symbols so that every symbol depends only on symbols of strictly smaller T?  Then all
    symbols of one T are independent of each other and can be decoded together."""
    return all(dx + a * dy + b * dc < 0 for dc, dy, dx in wavefront_dependencies(masks, num_layers))


def wavefront_coeffs(pc):
    """(a, b) of format 5 -- always WAVEFRONT_COEFFS = (2, 4) -- for a context model (probclass network object) whose own masks
    and layer count make it a valid order and whose width the wavefront decoder covers (k = 24); a ValueError otherwise."""
    a, b = WAVEFRONT_COEFFS
    if not wavefront_is_valid((pc.create_first_mask(), pc.create_other_mask()), pc.get_num_layers(), a, b):
        raise ValueError('wavefront order: T = x + {} y + {} c does not order the dependencies of this context model '
                         '({} layers)'.format(a, b, pc.get_num_layers()))
    k = getattr(pc, '_k', None)
    if k is None:
        k = int(pc.config.arch_param__k)
    if int(k) != 24:
        raise ValueError('wavefront order: the wavefront decoder covers context models of width k = 24, this one has k = {}'.format(k))
    return a, b


_ORDER_CACHE = {}


def wavefront_order(C, th, tw):
    """the coding order of format 5 for a (C, th, tw) tile: the flat raster indices c * th * tw + y * tw + x sorted by (T, c, y, x),
    T = x + 2 y + 4 c -> int64 array of C * th * tw elements.  Element 0 is index 0, the uncoded first symbol."""
    C, th, tw = int(C), int(th), int(tw)
    if C < 1 or th < 1 or tw < 1:
        raise ValueError('wavefront order: tile {} x {} x {} must be at least 1 in every extent'.format(C, th, tw))
    key = (C, th, tw)
    if key not in _ORDER_CACHE:
        a, b = WAVEFRONT_COEFFS
        c, y, x = np.meshgrid(np.arange(C), np.arange(th), np.arange(tw), indexing='ij')
        # raster order already is (c, y, x): a stable sort by T alone keeps it inside a front
        order = np.argsort((x + a * y + b * c).reshape(-1), kind='stable').astype(np.int64)
        order.setflags(write=False)
        if len(_ORDER_CACHE) > 64:
            _ORDER_CACHE.clear()
        _ORDER_CACHE[key] = order
    return _ORDER_CACHE[key]


def fill_symbol(centers):
    """the symbol that stands where nothing was decoded: the index of the centre of smallest magnitude, ties to the smallest index --
    what the quantiser emits where the importance map has masked a channel.  Concealment's fallback and the fill of a preview."""
    c = np.asarray(centers).reshape(-1)
    if c.size < 1:
        raise ValueError('fill symbol: no centres')
    return int(np.argmin(np.abs(c)))


def preview_symbols(symbols_chw, channels, fill):
    """the rule of a preview decode, on a full (C, h, w) symbol volume: a copy with [:channels] kept and [channels:] = fill."""
    out = np.array(symbols_chw, copy=True)
    out[int(channels):] = fill
    return out


def cap_channels(plane, C):
    """a cap plane that can be applied to symbols -> the (h, w) int64 plane of channels kept per cell, 0 .. C.  Every entry is an
    integer value in [0, C] or anything at or above C (+inf: no cap); a ValueError for a negative or NaN entry (as _check_level)
    and for a fractional one below C."""
    C = int(C)
    p = np.asarray(plane, dtype=np.float64)
    if p.ndim != 2:
        raise ValueError('cap plane of shape {}: expected (h, w)'.format(p.shape))
    if not bool((p >= 0).all()):                                     # (a NaN compares false)
        raise ValueError('cap {} is not in [0, +inf]'.format(float(p[~(p >= 0)].flat[0])))
    low = np.minimum(p, C)
    if not bool((low == np.floor(low)).all()):
        raise ValueError('cap {:g} is not an integer: a fractional cap rescales z and needs the bottleneck, so it belongs to compress '
                         'from the image; symbols take the integer levels 0 .. C = {}'.format(float(low[low != np.floor(low)].flat[0]), C))
    return low.astype(np.int64)


def cap_symbols(symbols_chw, plane, fill):
    """an integer cap applied to a (C, h, w) symbol volume: a copy with out[c, y, x] = symbols[c, y, x] if c < plane[y, x] else fill.
    plane: (h, w), as cap_channels takes it.  This is what the quantiser writes under that cap (an integer level cuts at a channel
    plane and leaves the channels below it as they are), so a file can be capped without its image: with a constant plane K it is
    preview_symbols(symbols, K, fill)."""
    sym = np.asarray(symbols_chw)
    if sym.ndim != 3:
        raise ValueError('cap_symbols: a (C, h, w) symbol volume is expected, got shape {}'.format(sym.shape))
    keep = cap_channels(plane, sym.shape[0])
    if keep.shape != sym.shape[1:]:
        raise ValueError('cap plane of shape {} for a symbol volume of {} x {} cells'.format(keep.shape, sym.shape[1], sym.shape[2]))
    out = np.array(sym, copy=True)
    out[np.arange(sym.shape[0])[:, None, None] >= keep[None]] = fill
    return out


def check_channels(channels, C):
    """the channels argument of the decompress calls: None (all of them) or an integer in 1 .. C; else a ValueError naming C"""
    if channels is None:
        return None
    if isinstance(channels, (bool, np.bool_)) or not isinstance(channels, (int, np.integer)) or not 1 <= int(channels) <= int(C):
        raise ValueError('channels = {!r}: a preview decodes an integer number of channels in 1 .. C = {}'.format(channels, int(C)))
    return int(channels)


def _below(m, h, w):
    """the number of (y, x), 0 <= y < h, 0 <= x < w, with x + 2 y <= m"""
    if m < 0:
        return 0
    Y = min(h - 1, m // 2)                                   # rows with a position at all; row y has min(w, m - 2 y + 1)
    full = min(max((m + 1 - w) // 2 + 1, 0), Y + 1)          # rows 0 .. full - 1 are whole
    rest = Y + 1 - full
    return full * w + rest * (m + 1) - (Y * (Y + 1) - full * (full - 1))


def wavefront_prefix_count(C, h, w, channels):
    """how many symbols of wavefront_order(C, h, w) a decoder steps through for the first `channels` channels: those with
    T = x + 2 y + 4 c <= (w - 1) + 2 (h - 1) + 4 (channels - 1), the front of that part's last symbol.  They are a prefix of the
    order (it is sorted by T first) and hold every symbol of the channels below `channels`; the uncoded first symbol counts."""
    C, h, w, channels = int(C), int(h), int(w), int(channels)
    if C < 1 or h < 1 or w < 1 or not 1 <= channels <= C:
        raise ValueError('wavefront prefix: tile {} x {} x {}, {} channels'.format(C, h, w, channels))
    T = (w - 1) + 2 * (h - 1) + 4 * (channels - 1)
    return sum(_below(T - 4 * c, h, w) for c in range(C))


def check_depth_block(depth_block, C):
    """the block side B of format 10: an integer in 1 .. 255, for a volume of at most 255 channels (a depth is one byte); else a
    ValueError naming the cause -> int"""
    if isinstance(depth_block, (bool, np.bool_)) or not isinstance(depth_block, (int, np.integer)) or not 1 <= int(depth_block) <= 255:
        raise ValueError('depth block = {!r}: the blocks of a depth plane are B x B cells with an integer B in 1 .. 255'.format(depth_block))
    if int(C) > 255:
        raise ValueError('depth-mapped tiles store a depth in one byte: C = {} is above 255'.format(int(C)))
    return int(depth_block)


def depth_plane(symbols_chw, fill, B):
    """the depth plane of a (C, h, w) tile: uint8 (ceil(h / B), ceil(w / B)); a block's entry is 0 if every symbol of its cells is
    `fill`, else 1 + the largest channel that holds another symbol in any of its cells.  Blocks are B x B cells counted from the
    tile's corner, ragged at the far edges."""
    sym = np.asarray(symbols_chw)
    if sym.ndim != 3:
        raise ValueError('depth_plane: a (C, h, w) symbol volume is expected, got shape {}'.format(sym.shape))
    C, h, w = sym.shape
    B = check_depth_block(B, C)
    cell = ((sym != fill) * (np.arange(C, dtype=np.int64) + 1)[:, None, None]).max(axis=0)     # per cell: 1 + deepest channel, 0: none
    nby, nbx = -(-h // B), -(-w // B)
    padded = np.zeros((nby * B, nbx * B), dtype=np.int64)
    padded[:h, :w] = cell
    return padded.reshape(nby, B, nbx, B).max(axis=(1, 3)).astype(np.uint8)


def _depth_per_cell(C, th, tw, depth, B):
    """the depth plane spread over the cells of a (th, tw) tile, clamped to C -> int64 (th, tw)"""
    C, th, tw = int(C), int(th), int(tw)
    B = check_depth_block(B, C)
    d = np.asarray(depth)
    if d.shape != (-(-th // B), -(-tw // B)):
        raise ValueError('depth plane of shape {} for a {} x {} tile in blocks of {}: expected {} x {}'.format(
            d.shape, th, tw, B, -(-th // B), -(-tw // B)))
    return np.minimum(np.repeat(np.repeat(d.astype(np.int64), B, axis=0), B, axis=1)[:th, :tw], C)


def depth_live(C, th, tw, depth, B):
    """the live positions of a (C, th, tw) tile under a depth plane: bool (C, th, tw), [c, y, x] = c < depth[y // B][x // B]"""
    return np.arange(int(C))[:, None, None] < _depth_per_cell(C, th, tw, depth, B)[None]


def depth_live_mask(C, th, tw, depth, B):
    """the keep-mask of format 10 in coding order: bool of C * th * tw elements, element i says whether position
    wavefront_order(C, th, tw)[i] is live.  The coded sequence of a tile is its wavefront order with the dead positions left out --
    and element 0, the first position, uncoded as ever; a dead position holds the fill symbol, the first one included."""
    return depth_live(C, th, tw, depth, B).reshape(-1)[wavefront_order(C, th, tw)]


def depth_front_steps(th, tw, dmax):
    """the steps of the front sweep that decodes a (., th, tw) tile whose deepest block is dmax: the fronts T = 7 .. (tw + 3) +
    2 (th + 3) + 4 (dmax + 3) of the padded volume, none for a tile that holds nothing.  dmax = C is the sweep of format 5."""
    return 0 if int(dmax) < 1 else (int(tw) + 3) + 2 * (int(th) + 3) + 4 * (int(dmax) + 3) - 6


def split_depth_stream(stream, C, th, tw, B, tile=None):
    """a tile's stream of format 10 -> (depth plane uint8 (nby, nbx), the coder's bytes); a ValueError naming the tile for a stream
    shorter than its plane and for a depth above C"""
    nby, nbx = -(-int(th) // B), -(-int(tw) // B)
    where = '' if tile is None else ' of tile {}'.format(tile)
    if len(stream) < nby * nbx:
        raise ValueError('stream{} holds {} bytes, its depth plane of {} x {} blocks alone has {}'.format(where, len(stream), nby, nbx, nby * nbx))
    depth = np.frombuffer(bytes(stream[:nby * nbx]), dtype=np.uint8).reshape(nby, nbx)
    if depth.size and int(depth.max()) > int(C):
        raise ValueError('depth plane{} holds {}, above C = {}'.format(where, int(depth.max()), int(C)))
    return depth, bytes(stream[nby * nbx:])


def check_rans_lanes(lanes):
    """the number W of interleaved coders of format 12: one of RANS_LANES; else a ValueError -> int"""
    if isinstance(lanes, (bool, np.bool_)) or not isinstance(lanes, (int, np.integer)) or int(lanes) not in RANS_LANES:
        raise ValueError('lanes = {!r}: a tile of format 12 is coded by W interleaved coders, W one of {}'.format(
            lanes, ', '.join(str(w) for w in RANS_LANES)))
    return int(lanes)


RANS_MAX_TOTAL = (1 << 30) + 2                                       # arithmetic_coding.MAX_TOTAL: the limit of every coder here


def rans_table(freqs_row):
    """the rANS coder's table of one context, an integer function of the arithmetic coder's integer table f (pc_table_row): with
    T = sum f, M = 2^16, g_j = max(1, f_j (M - L) // T), and the deficit M - sum g, which is >= 1, added to the first entry with the
    largest f_j -> int64 (L,), sum exactly M, every entry >= 1.  1 <= L <= 16.  The total is not looked at: T > RANS_MAX_TOTAL is
    status 1 of the coders, as for every coder here."""
    f = [int(v) for v in np.asarray(freqs_row).reshape(-1)]
    L = len(f)
    if not 1 <= L <= 16 or min(f) < 1:
        raise ValueError('rans_table: a table row has 1 .. 16 frequencies, each >= 1, got {!r}'.format(f))
    T = sum(f)
    g = [max(1, fj * (RANS_M - L) // T) for fj in f]
    g[f.index(max(f))] += RANS_M - sum(g)
    return np.asarray(g, dtype=np.int64)


def _rans_slots(C, th, tw):
    """(t, e) of every position of a (C, th, tw) tile: int64 (C, th, tw) each"""
    c, y, x = np.meshgrid(np.arange(C, dtype=np.int64), np.arange(th, dtype=np.int64), np.arange(tw, dtype=np.int64), indexing='ij')
    t = x + 2 * y + 4 * c
    iw = min(th, (tw + 1) // 2)
    c_lo = np.maximum(0, -((-(t - (tw - 1) - 2 * (th - 1))) // 4))
    y_lo = np.maximum(0, -((-(t - 4 * c - (tw - 1))) // 2))
    return t, (c - c_lo) * iw + (y - y_lo)


def rans_slot(C, th, tw, c, y, x):
    """the candidate index e of position (c, y, x) on its front t = x + 2 y + 4 c -- the enumeration of the front decoder: channels
    from the first that has a position on the front, iw = min(th, (tw + 1) // 2) slots each, rows from the first that has one.  The
    positions of a front have distinct e, ascending in (c, y, x) order; an e that is no position is a hole.  Coder = e mod W, round =
    (t, e div W)."""
    C, th, tw, c, y, x = (int(v) for v in (C, th, tw, c, y, x))
    if not (0 <= c < C and 0 <= y < th and 0 <= x < tw):
        raise ValueError('rans_slot: ({}, {}, {}) is no position of a {} x {} x {} tile'.format(c, y, x, C, th, tw))
    t = x + 2 * y + 4 * c
    iw = min(th, (tw + 1) // 2)
    c_lo = max(0, -((-(t - (tw - 1) - 2 * (th - 1))) // 4))
    y_lo = max(0, -((-(t - 4 * c - (tw - 1))) // 2))
    return (c - c_lo) * iw + (y - y_lo)


_RANS_CACHE = {}


def rans_rounds(C, th, tw, W):
    """the rounds of format 12 for a (C, th, tw) tile coded by W coders: int64 (R, W), [r, l] = the flat raster index of the position
    coder l codes in round r, -1 for a hole and for the uncoded first position.  Rounds are ordered by (t, e div W); rounds that
    hold only -1 are dropped (they cost no bytes on either side)."""
    C, th, tw, W = int(C), int(th), int(tw), check_rans_lanes(W)
    if C < 1 or th < 1 or tw < 1:
        raise ValueError('rans rounds: tile {} x {} x {} must be at least 1 in every extent'.format(C, th, tw))
    key = (C, th, tw, W)
    if key not in _RANS_CACHE:
        t, e = _rans_slots(C, th, tw)
        t, e = t.reshape(-1)[1:], e.reshape(-1)[1:]                  # without the first position
        span = int(e.max()) // W + 1 if e.size else 1
        keys, inverse = np.unique(t * span + e // W, return_inverse=True)
        rounds = np.full((len(keys), W), -1, dtype=np.int64)
        rounds[inverse.reshape(-1), e % W] = np.arange(1, C * th * tw, dtype=np.int64)
        rounds.setflags(write=False)
        if len(_RANS_CACHE) > 64:
            _RANS_CACHE.clear()
        _RANS_CACHE[key] = rounds
    return _RANS_CACHE[key]


def rans_encode(freqs, symbols, W):
    """the tile stream of format 12.  freqs: (R W, L) rows of the arithmetic coder's table, symbols: (R W,) in round order (element
    r W + l is coder l's of round r; -1: a hole, its row is not looked at) -> bytes: the W final states ('<I', coder l at byte 4 l),
    then the 16-bit words ('<H') in the order the decoder takes them -- rounds ascending, within a round the coders that need one
    in ascending order.  State x in [2^16, 2^32), initially 2^16; a step with (g, cg) of rans_table: if x >= g << 16, emit x & 0xffff
    and x >>= 16; then x = ((x // g) << 16) + x % g + cg.  The rounds are coded backwards.  A ValueError for a total above
    RANS_MAX_TOTAL (status 1 of the device) and for a symbol outside [0, L) (status 3)."""
    W = check_rans_lanes(W)
    sym = np.asarray(symbols, dtype=np.int64).reshape(-1)
    fr = np.asarray(freqs, dtype=np.int64)
    fr = fr.reshape(sym.size, -1) if sym.size else np.zeros((0, 1), np.int64)
    if sym.size % W:
        raise ValueError('rans_encode: {} symbols are no whole rounds of {} coders'.format(sym.size, W))
    L = fr.shape[1]
    state = [RANS_M] * W
    words = []                                                       # backwards
    for i in range(sym.size - 1, -1, -1):
        s = int(sym[i])
        if s == -1:
            continue
        if not 0 <= s < L:
            raise ValueError('rans_encode: symbol {} outside [0, {})'.format(s, L))
        if int(fr[i].sum()) > RANS_MAX_TOTAL:
            raise ValueError('Cannot code symbol because total is too large')
        row = rans_table(fr[i])
        g, cg = int(row[s]), int(row[:s].sum())
        x = state[i % W]
        if x >= g << 16:
            words.append(x & 0xffff)
            x >>= 16
        state[i % W] = ((x // g) << 16) + x % g + cg
    return struct.pack('<{}I'.format(W), *state) + struct.pack('<{}H'.format(len(words)), *reversed(words))


def rans_decode(data, rounds, W, freqs_of, out, full=True, stop=None):
    """the mirror of rans_encode.  rounds: (R, W) indices into `out` as rans_rounds gives them; freqs_of(out, index) -> the table
    row of that position, asked for when every earlier round is in `out` (a flat int64 array, written in place).  A step: s = x &
    0xffff, the symbol with cg <= s < cg + g, x = g (x >> 16) + s - cg, and if x < 2^16, x = (x << 16) | the next word.  Past its
    end the stream reads as zeros.  stop: the number of rounds to decode (a preview).  -> status: 0; 1 = a total above
    RANS_MAX_TOTAL (decoding goes on); 4 = (full decodes only) some coder's state is not 2^16 at the end or the stream does not end
    where the coders' run ends, 4 W + 2 words != len(data)."""
    W = check_rans_lanes(W)
    data = bytes(data)

    def byte(i):
        return data[i] if i < len(data) else 0

    state = [byte(4 * l) | byte(4 * l + 1) << 8 | byte(4 * l + 2) << 16 | byte(4 * l + 3) << 24 for l in range(W)]
    taken, status = 0, 0
    rounds = np.asarray(rounds)
    R = len(rounds) if stop is None else int(stop)
    for r in range(R):
        syms = []
        for l in range(W):
            i = int(rounds[r, l])
            if i < 0:
                continue
            f = np.asarray(freqs_of(out, i), dtype=np.int64)
            if int(f.sum()) > RANS_MAX_TOTAL:
                status |= 1
            cum = np.concatenate([[0], np.cumsum(rans_table(f))])
            x = state[l]
            s = x & 0xffff
            k = int(np.searchsorted(cum, s, side='right')) - 1
            x = int(cum[k + 1] - cum[k]) * (x >> 16) + s - int(cum[k])
            if x < RANS_M:
                x = x << 16 | byte(4 * W + 2 * taken) | byte(4 * W + 2 * taken + 1) << 8
                taken += 1
            state[l] = x
            syms.append((i, k))
        for i, k in syms:                                            # a round's positions do not see each other
            out[i] = k
    if full and stop is None and (any(x != RANS_M for x in state) or 4 * W + 2 * taken != len(data)):
        status |= 4
    return status


# ---- rate-aware symbol choice at encode (compress(rdo=...), IC_PC_DECODE_RDO): the rule of one position, the host's statement ----

def ilog2_q16(v):
    """log2 v in 2^-16 units for an integer 1 <= v < 2^32, computed in integers only: e = the position of the top bit,
    m = v << (31 - e), r = e, then 16 times m = (m m) >> 31, r = 2 r, and if m >= 2^32: m >>= 1, r |= 1.  Every intermediate fits
    64 unsigned bits; exact on powers of two; what the device computes bit for bit."""
    v = int(v)
    if not 1 <= v < (1 << 32):
        raise ValueError('ilog2_q16: {} is outside 1 .. 2^32 - 1'.format(v))
    e = v.bit_length() - 1
    m, r = v << (31 - e), e
    for _ in range(16):
        m, r = (m * m) >> 31, r << 1
        if m >> 32:
            m, r = m >> 1, r | 1
    return r


def check_rdo(rdo):
    """a lambda of compress(rdo=...): a number with 0 <= lambda < inf; else a ValueError -> float"""
    if isinstance(rdo, (bool, np.bool_)) or not isinstance(rdo, (int, float, np.integer, np.floating)) or not 0.0 <= float(rdo) < float('inf'):
        raise ValueError('rdo = {!r}: lambda is a number with 0 <= lambda < inf (0: the quantiser\'s own symbols)'.format(rdo))
    return float(rdo)


def rdo_lambda_q(lam):
    """lambda, in units of the quantiser's key per bit -> Lambda = lambda * 1e7 / 65536 (float64): the factor on a rate in 2^-16
    bits beside the key k = fl32(1e7 fl32(t t))"""
    return check_rdo(lam) * 1e7 / 65536.0


def rdo_choose(z, freqs_row, centers, lam_q, rated=True):
    """the symbol of one position -> (symbol, status): the first j that attains min_j cost_j under `<`,
    cost_j = float64(k_j) + lam_q * float64(R_j) (one rounded multiply, one rounded add), k_j = fl32(1e7 fl32(t t)) with
    t = fl32(|z - c_j|), R_j = ilog2_q16(T) - ilog2_q16(f_j) over the coder's table row f, T = sum f.  rated=False (a tile's first
    position, which every format stores raw) and a row whose total exceeds RANS_MAX_TOTAL (status 1): all R_j = 0.  lam_q = 0 is the
    hard quantiser's symbol; a NaN cost never wins."""
    c = np.asarray(centers, dtype=np.float32).reshape(-1)
    L, status = len(c), 0
    R = [0] * L
    if rated:
        f = [int(v) for v in np.asarray(freqs_row).reshape(-1)]
        if len(f) != L:
            raise ValueError('rdo_choose: a table row of {} entries for {} centres'.format(len(f), L))
        T = sum(f)
        if T > RANS_MAX_TOTAL:
            status = 1
        else:
            lT = ilog2_q16(T)
            R = [lT - ilog2_q16(fj) for fj in f]
    with np.errstate(over='ignore', invalid='ignore'):
        t = np.abs(np.float32(z) - c)
        k = (np.float32(1e7) * (t * t).astype(np.float32)).astype(np.float32).astype(np.float64)
        cost = k + np.float64(lam_q) * np.asarray(R, dtype=np.float64)
    best, sym = float('inf'), 0
    for j in range(L):
        if float(cost[j]) < best:
            best, sym = float(cost[j]), j
    return sym, status


def rdo_record_bytes(C, th, tw):
    """the length of a tile's record: Lambda, then C th tw float32"""
    return 8 + 4 * int(C) * int(th) * int(tw)


def rdo_record(lam_q, z_chw):
    """a tile's record as the chooser reads it: Lambda as a little-endian f64, then the tile's z as float32 in (c, y, x) order.
    The host's statement of the layout, for callers of the C ABI and for the tests: no path of this package builds records on the
    host (PredictionNetwork.choose_tiles_batch gathers them on the device)"""
    z = np.ascontiguousarray(z_chw, dtype='<f4')
    if z.ndim != 3:
        raise ValueError('rdo_record: z is a (C, th, tw) array, got shape {}'.format(z.shape))
    return struct.pack('<d', float(lam_q)) + z.tobytes()


def check_rdo_record(off, nbytes, C, th, tw):
    """what the entry asks of a record's place in the buffer: an offset that is a multiple of 8, the exact length.  The host's
    statement of the entry's own argument checks (IC_ERR_ARG), like rdo_record for callers of the C ABI and for the tests"""
    if int(off) % 8 != 0:
        raise ValueError('record at offset {}: not a multiple of 8'.format(off))
    if int(nbytes) != rdo_record_bytes(C, th, tw):
        raise ValueError('record of {} bytes for a {} x {} x {} tile: expected {}'.format(nbytes, C, th, tw, rdo_record_bytes(C, th, tw)))


def rdo_is_sequence(rdo):
    """is this rdo argument one lambda per tile (a list, a tuple, an array of at least one dimension) and not one number?"""
    return isinstance(rdo, (list, tuple)) or (isinstance(rdo, np.ndarray) and rdo.ndim > 0)


def rdo_tile_lambdas(rdo, ntiles):
    """compress's rdo argument for a volume of ntiles tiles -> [lambda per tile in tile_grid order]: a number serves every tile, a
    sequence has one entry per tile"""
    if not rdo_is_sequence(rdo):
        return [check_rdo(rdo.item() if isinstance(rdo, np.ndarray) else rdo)] * int(ntiles)
    lams = [check_rdo(v) for v in list(rdo)]
    if len(lams) != int(ntiles):
        raise ValueError('rdo: {} lambdas for {} tiles'.format(len(lams), ntiles))
    return lams


def chunk_tiles(tile_shapes, need, budget):
    """cut a list of tiles [(th, tw)] into consecutive chunks [(start, stop)] for a decoder whose workspace grows with the number of
    tiles of a call: need(th_max, tw_max, ntiles) -> bytes for a chunk of ntiles tiles, the largest th x tw.  Greedy, order kept:
    every tile is in exactly one chunk and need(chunk) <= budget for every chunk; a tile that does not fit alone is a ValueError."""
    chunks, start = [], 0
    while start < len(tile_shapes):
        th_max, tw_max = int(tile_shapes[start][0]), int(tile_shapes[start][1])
        if need(th_max, tw_max, 1) > budget:
            raise ValueError('tile {} of {} x {} needs a workspace of {} bytes, the budget is {}'.format(
                start, th_max, tw_max, need(th_max, tw_max, 1), budget))
        stop = start + 1
        while stop < len(tile_shapes):
            a, b = max(th_max, int(tile_shapes[stop][0])), max(tw_max, int(tile_shapes[stop][1]))
            if need(a, b, stop + 1 - start) > budget:
                break
            th_max, tw_max, stop = a, b, stop + 1
        chunks.append((start, stop))
        start = stop
    return chunks


def list_dir_jobs(in_dir, out_dir, command):
    """the files a -dir command works on: [(input path, output path)] sorted by file name.  compress-dir: every *.png / *.jpg of
    in_dir -> out_dir/<stem>.icf; decompress-dir: every *.icf -> out_dir/<stem>.png.  Two inputs with one stem (a.png, a.jpg) would
    write one output: a ValueError, as is a missing directory or one without such files."""
    exts, out_ext = {'compress-dir': (('.png', '.jpg'), '.icf'), 'decompress-dir': (('.icf',), '.png'),
                     'transcode-dir': (('.icf',), '.icf')}[command]
    if not os.path.isdir(in_dir):
        raise ValueError('{}: {!r} is not a directory'.format(command, in_dir))
    names = sorted(n for n in os.listdir(in_dir)
                   if os.path.splitext(n)[1].lower() in exts and os.path.isfile(os.path.join(in_dir, n)))
    if not names:
        raise ValueError('{}: no {} file in {!r}'.format(command, ' / '.join('*' + e for e in exts), in_dir))
    jobs, seen = [], {}
    for n in names:
        stem = os.path.splitext(n)[0]
        if stem in seen:
            raise ValueError('{}: {} and {} would both be written to {}{}'.format(command, seen[stem], n, stem, out_ext))
        seen[stem] = n
        jobs.append((os.path.join(in_dir, n), os.path.join(out_dir, stem + out_ext)))
    return jobs


def _tiled_head(version, ae_name, pc_name, H, W, C, h, w, L, resolution, fingerprint, th, tw, rows, n, extra=None):
    a, p = ae_name.encode('utf-8'), pc_name.encode('utf-8')
    return b''.join([
        MAGIC, struct.pack('<H', version),
        struct.pack('<H', len(a)), a, struct.pack('<H', len(p)), p,
        struct.pack('<II', H, W), struct.pack('<HII', C, h, w), struct.pack('<H', L),
        struct.pack('<d', float(resolution)), struct.pack('<I', fingerprint & 0xffffffff),
        struct.pack('<HH', th, tw), b'' if extra is None else struct.pack('<H', extra), struct.pack('<I', len(rows))] +
        rows + [struct.pack('<Q', n)])


def _build_tiled(version, ae_name, pc_name, H, W, C, h, w, L, resolution, fingerprint, th, tw, first_syms, streams, extra=None):
    """formats 2, 4, 5, 10 and 12: the head, its CRC if the format has one, the streams, the CRC over the file"""
    row = FORMATS[version]
    streams = [bytes(b) for b in streams]
    assert len(first_syms) == len(streams)
    if row.extra is not None:
        extra = row.check_extra(extra, C)
    head = _tiled_head(version, ae_name, pc_name, H, W, C, h, w, L, resolution, fingerprint, th, tw,
                       [struct.pack('<HII', f, len(b), zlib.crc32(b) & 0xffffffff) if row.checked else struct.pack('<HI', f, len(b))
                        for f, b in zip(first_syms, streams)], sum(len(b) for b in streams), extra)
    body = head + (struct.pack('<I', zlib.crc32(head) & 0xffffffff) if row.checked else b'') + b''.join(streams)
    return body + struct.pack('<I', zlib.crc32(body) & 0xffffffff)


def build_tiled_container(ae_name, pc_name, H, W, C, h, w, L, resolution, fingerprint, th, tw, first_syms, streams):
    """format 2: first_syms / streams per tile in the order of tile_grid(h, w, th, tw)."""
    return _build_tiled(FORMAT_VERSION_TILED, ae_name, pc_name, H, W, C, h, w, L, resolution, fingerprint, th, tw, first_syms, streams)


def build_checked_container(ae_name, pc_name, H, W, C, h, w, L, resolution, fingerprint, th, tw, first_syms, streams):
    """format 4: format 2 with a CRC-32 per stream in the tile table and a CRC-32 over the header behind the payload length."""
    return _build_tiled(FORMAT_VERSION_CHECKED, ae_name, pc_name, H, W, C, h, w, L, resolution, fingerprint, th, tw, first_syms, streams)


def build_wavefront_container(ae_name, pc_name, H, W, C, h, w, L, resolution, fingerprint, th, tw, first_syms, streams):
    """format 5: the bytes of format 4 with version 5; streams[t] codes tile t's symbols in wavefront_order(C, th', tw')."""
    return _build_tiled(FORMAT_VERSION_WAVEFRONT, ae_name, pc_name, H, W, C, h, w, L, resolution, fingerprint, th, tw, first_syms, streams)


def build_depth_container(ae_name, pc_name, H, W, C, h, w, L, resolution, fingerprint, th, tw, depth_block, first_syms, streams):
    """format 10: the layout of formats 4 / 5 with the depth block B as one '<H' behind the tile extent; streams[t] is tile t's depth
    plane (depth_plane of its symbols, row-major bytes) followed by the range coder's bytes over its live positions
    (depth_live_mask), and the tile's CRC covers both."""
    return _build_tiled(FORMAT_VERSION_DEPTH, ae_name, pc_name, H, W, C, h, w, L, resolution, fingerprint, th, tw, first_syms, streams,
                        depth_block)


def build_rans_container(ae_name, pc_name, H, W, C, h, w, L, resolution, fingerprint, th, tw, lanes, first_syms, streams):
    """format 12: the layout of format 10 with the number of coders W as the '<H' behind the tile extent; streams[t] is tile t's
    rANS stream (rans_encode over the rounds rans_rounds of its own extent), and the tile's CRC covers it."""
    return _build_tiled(FORMAT_VERSION_RANS, ae_name, pc_name, H, W, C, h, w, L, resolution, fingerprint, th, tw, first_syms, streams, lanes)


def default_layer_ends(C):
    """the layer ends of --progressive / layers='default': [max(1, C // 8), C // 4, C // 2, C] with repeats and zeros dropped --
    4, 8, 16, 32 for C = 32; increasing, at most four, the last one C"""
    C = int(C)
    if C < 1:
        raise ValueError('layer ends: C = {} is not at least 1'.format(C))
    return sorted(set(e for e in (max(1, C // 8), C // 4, C // 2, C) if e > 0))


def check_layer_ends(layer_ends, C):
    """layer ends e_0 < e_1 < .. < e_{G-1} = C with 1 <= G <= 16 and e_0 >= 1 -> list of int; else a ValueError naming the cause"""
    try:
        ends = [int(e) for e in layer_ends]
        whole = all(not isinstance(e, (bool, np.bool_)) and int(e) == e for e in layer_ends)
    except (TypeError, ValueError):
        raise ValueError('layer ends {!r} are not a sequence of integers'.format(layer_ends))
    if not whole:
        raise ValueError('layer ends {!r} are not a sequence of integers'.format(layer_ends))
    if not 1 <= len(ends) <= MAX_LAYERS:
        raise ValueError('layer count G = {} is outside 1 .. {}'.format(len(ends), MAX_LAYERS))
    if ends[0] < 1 or any(b <= a for a, b in zip(ends, ends[1:])):
        raise ValueError('layer ends {} are not increasing from at least 1'.format(ends))
    if ends[-1] != int(C):
        raise ValueError('last layer end {} is not C = {}: the layers must hold every channel'.format(ends[-1], int(C)))
    return ends


def front_layer_cuts(C, th, tw, layer_ends):
    """the cuts of format 8 for a (C, th, tw) tile: [n_0 < n_1 < .. < n_{G-1} = C th tw], n_g = wavefront_prefix_count(C, th, tw, e_g).
    Segment g holds the symbols of wavefront_order(C, th, tw) with index in [n_{g-1}, n_g), n_{-1} = 0 (index 0 is the uncoded first
    symbol): all symbols up to the front of the last symbol of channel e_g - 1, so segments 0 .. g hold every symbol of the channels
    below e_g -- and the symbols of later channels that share those fronts.  e_0 = 1 on a 1 x 1 tile: n_0 = 1, an empty segment 0."""
    ends = check_layer_ends(layer_ends, C)
    return [wavefront_prefix_count(C, th, tw, e) for e in ends]


def build_front_layered_container(ae_name, pc_name, H, W, C, h, w, L, resolution, fingerprint, th, tw, first_syms, layer_ends, segments):
    """format 8: the bytes of format 6 with version 8; segments[g][t] codes tile t's symbols of wavefront_order(C, th', tw') between
    the cuts front_layer_cuts(C, th', tw', layer_ends)[g - 1] and [g]."""
    return build_layered_container(ae_name, pc_name, H, W, C, h, w, L, resolution, fingerprint, th, tw, first_syms, layer_ends, segments,
                                   version=FORMAT_VERSION_FRONTS)


def build_layered_container(ae_name, pc_name, H, W, C, h, w, L, resolution, fingerprint, th, tw, first_syms, layer_ends, segments,
                            version=FORMAT_VERSION_LAYERED):
    """format 6: segments[g][t] = the bytes of layer g of tile t (tiles in the order of tile_grid(h, w, th, tw))."""
    assert version in _LAYERED_VERSIONS
    ends = check_layer_ends(layer_ends, C)
    segments = [[bytes(b) for b in layer] for layer in segments]
    assert len(segments) == len(ends) and all(len(layer) == len(first_syms) for layer in segments)
    front = _tiled_head(version, ae_name, pc_name, H, W, C, h, w, L, resolution, fingerprint, th, tw, [b''] * len(first_syms), 0)[:-8]
    flat = [b for layer in segments for b in layer]
    head = b''.join([front, struct.pack('<H', len(ends)), struct.pack('<{}H'.format(len(ends)), *ends),
                     struct.pack('<{}H'.format(len(first_syms)), *first_syms)] +
                    [struct.pack('<II', len(b), zlib.crc32(b) & 0xffffffff) for b in flat] + [struct.pack('<Q', sum(len(b) for b in flat))])
    body = head + struct.pack('<I', zlib.crc32(head) & 0xffffffff) + b''.join(flat)
    return body + struct.pack('<I', zlib.crc32(body) & 0xffffffff)


def build_container(ae_name, pc_name, H, W, C, h, w, L, first_sym, resolution, fingerprint, payload):
    a, p = ae_name.encode('utf-8'), pc_name.encode('utf-8')
    head = b''.join([
        MAGIC, struct.pack('<H', FORMAT_VERSION),
        struct.pack('<H', len(a)), a, struct.pack('<H', len(p)), p,
        struct.pack('<II', H, W), struct.pack('<HII', C, h, w), struct.pack('<HH', L, first_sym),
        struct.pack('<d', float(resolution)), struct.pack('<I', fingerprint & 0xffffffff),
        struct.pack('<Q', len(payload))])
    body = head + bytes(payload)
    return body + struct.pack('<I', zlib.crc32(body) & 0xffffffff)


class _Reader(object):
    """bounds-checked cursor: a length field is never believed beyond the bytes that are there."""

    def __init__(self, data):
        self.data, self.pos = data, 0

    def take(self, n, what):
        if n < 0 or self.pos + n > len(self.data):
            raise ValueError('truncated file: {} needs {} bytes at offset {}, {} left'.format(
                what, n, self.pos, len(self.data) - self.pos))
        out = self.data[self.pos:self.pos + n]
        self.pos += n
        return out

    def unpack(self, fmt, what):
        return struct.unpack(fmt, self.take(struct.calcsize(fmt), what))


def parse_container(data):
    """bytes -> the container type of the file's version (FORMATS): Container (1), TiledContainer (2), CheckedContainer (4),
    WavefrontContainer (5), LayeredContainer (6 and 8), DepthContainer (10) or RansContainer (12).
    Order: size, magic, version, CRC over the whole file -- only then are the header's lengths read, each against the bytes that
    remain; the payload length must equal exactly what is left before the CRC.  The formats with checksums in addition: the header
    CRC and every stream's or segment's CRC; formats 10 and 12: the extra header field and every stream's own layout."""
    data = bytes(data)
    if len(data) < _MIN_SIZE:
        raise ValueError('truncated file: {} bytes, the smallest container has {}'.format(len(data), _MIN_SIZE))
    if data[:4] != MAGIC:
        raise ValueError('wrong magic {!r}: not a codec file (expected {!r})'.format(data[:4], MAGIC))
    version, = struct.unpack('<H', data[4:6])
    if version not in FORMATS:
        raise ValueError(_unsupported(version))
    stored, = struct.unpack('<I', data[-4:])
    actual = zlib.crc32(data[:-4]) & 0xffffffff
    if stored != actual:
        raise ValueError('CRC mismatch: file says {:08x}, content gives {:08x} (corrupt or truncated file)'.format(stored, actual))
    r = _Reader(data[:-4])
    ae_name, pc_name, H, W, C, h, w = _parse_front(r)
    if FORMATS[version].layered:
        return _parse_layered(r, ae_name, pc_name, H, W, C, h, w, strict=True, version=version)[0]
    if version != FORMAT_VERSION:
        return _parse_tiled(r, version, ae_name, pc_name, H, W, C, h, w)
    L, first_sym = r.unpack('<HH', 'L and first symbol')
    resolution, = r.unpack('<d', 'frequency resolution')
    fingerprint, = r.unpack('<I', 'model fingerprint')
    n, = r.unpack('<Q', 'payload length')
    left = len(r.data) - r.pos
    if n != left:
        raise ValueError('payload length {} does not equal the {} bytes that remain in the file'.format(n, left))
    return Container(version, ae_name, pc_name, H, W, C, h, w, L, first_sym, resolution, fingerprint, r.take(n, 'payload'))


def _unsupported(version):
    return ('unsupported format version {} (this codec reads versions {}, {} and {}) and the wavefront version {} and the layered '
            'version {} and the front-layered version {}'.format(version, FORMAT_VERSION, FORMAT_VERSION_TILED, FORMAT_VERSION_CHECKED,
                                                                 FORMAT_VERSION_WAVEFRONT, FORMAT_VERSION_LAYERED, FORMAT_VERSION_FRONTS))


def _parse_front(r):
    """what every format begins with: magic and version (checked by the caller), the two names, the image and volume shapes"""
    r.take(6, 'magic and version')
    ae_name = r.take(r.unpack('<H', 'ae config name length')[0], 'ae config name')
    pc_name = r.take(r.unpack('<H', 'pc config name length')[0], 'pc config name')
    try:
        ae_name, pc_name = ae_name.decode('utf-8'), pc_name.decode('utf-8')
    except UnicodeDecodeError:
        raise ValueError('config name is not UTF-8')
    H, W = r.unpack('<II', 'image size')
    C, h, w = r.unpack('<HII', 'symbol volume shape')
    return ae_name, pc_name, H, W, C, h, w


def _parse_tile_extent(r, h, w, has_extra=False):
    """L .. tile count, which every tiled format has -> (L, resolution, fingerprint, th, tw, ntiles, extra); extra: the field that
    stands behind the tile extent in a format-10 / format-12 header, else None"""
    L, = r.unpack('<H', 'L')
    resolution, = r.unpack('<d', 'frequency resolution')
    fingerprint, = r.unpack('<I', 'model fingerprint')
    th, tw = r.unpack('<HH', 'tile extent')
    extra = r.unpack('<H', 'depth block')[0] if has_extra else None
    ntiles, = r.unpack('<I', 'tile count')
    if th == 0 or tw == 0:
        raise ValueError('tile extent {} x {}: a tile has at least one row and one column'.format(th, tw))
    if h < 1 or w < 1:
        raise ValueError('symbol volume {} x {} cannot be tiled'.format(h, w))
    expected = ((h + th - 1) // th) * ((w + tw - 1) // tw)
    if ntiles != expected:
        raise ValueError('tile count {} does not equal the {} tiles of a {} x {} volume cut into {} x {}'.format(
            ntiles, expected, h, w, th, tw))
    return L, resolution, fingerprint, th, tw, ntiles, extra


def _parse_tile_table(r, version, h, w):
    """L .. payload length of an unlayered tiled header, every length against the bytes that remain -> (L, resolution, fingerprint,
    th, tw, first_syms, lengths, crcs or None, n, extra as _parse_tile_extent gives it)"""
    checked = FORMATS[version].checked
    L, resolution, fingerprint, th, tw, ntiles, extra = _parse_tile_extent(r, h, w, FORMATS[version].extra is not None)
    row = 10 if checked else 6
    table = r.take(row * ntiles, 'tile table')            # against the bytes that remain, before anything of its size is built
    first_syms, lengths, crcs = [], [], [] if checked else None
    for t in range(ntiles):
        if checked:
            f, n_t, crc = struct.unpack_from('<HII', table, row * t)
            crcs.append(crc)
        else:
            f, n_t = struct.unpack_from('<HI', table, row * t)
        if f >= L:
            raise ValueError('first symbol {} of tile {} is not below L = {}'.format(f, t, L))
        first_syms.append(f)
        lengths.append(n_t)
    n, = r.unpack('<Q', 'payload length')
    if sum(lengths) != n:
        raise ValueError('stream lengths of the {} tiles sum to {}, the payload length is {}'.format(ntiles, sum(lengths), n))
    return L, resolution, fingerprint, th, tw, first_syms, lengths, crcs, n, extra


def _parse_tiled(r, version, ae_name, pc_name, H, W, C, h, w):
    """the rest of an unlayered tiled file after the symbol volume shape (the CRC over the file has been checked)."""
    L, resolution, fingerprint, th, tw, first_syms, lengths, crcs, n, extra = _parse_tile_table(r, version, h, w)
    if crcs is not None:
        end = r.pos
        stored, = r.unpack('<I', 'header CRC')
        actual = zlib.crc32(r.data[:end]) & 0xffffffff
        if stored != actual:
            raise ValueError('header CRC mismatch: file says {:08x}, the header gives {:08x}'.format(stored, actual))
    left = len(r.data) - r.pos
    if n != left:
        raise ValueError('payload length {} does not equal the {} bytes that remain in the file'.format(n, left))
    payload = r.take(n, 'payload')
    streams, pos = [], 0
    for n_t in lengths:
        streams.append(payload[pos:pos + n_t])
        pos += n_t
    c = FORMATS[version].container
    if crcs is None:
        return c(version, ae_name, pc_name, H, W, C, h, w, L, resolution, fingerprint, th, tw, first_syms, streams, payload)
    for t, (b, crc) in enumerate(zip(streams, crcs)):
        actual = zlib.crc32(b) & 0xffffffff
        if actual != crc:
            raise ValueError('stream CRC mismatch in tile {}: the table says {:08x}, the stream gives {:08x}'.format(t, crc, actual))
    if version == FORMAT_VERSION_DEPTH:
        B = extra
        if not 1 <= B <= 255 or C > 255:
            raise ValueError('depth block {} with C = {}: format 10 has blocks of 1 .. 255 cells and at most 255 channels'.format(B, C))
        for t, ((_, _, a, b), s) in enumerate(zip(tile_grid(h, w, th, tw), streams)):
            split_depth_stream(s, C, a, b, B, tile=t)     # a stream shorter than its plane, a depth above C: refused, naming the tile
    if version == FORMAT_VERSION_RANS:
        lanes = extra
        if lanes not in RANS_LANES:
            raise ValueError('{} coders per tile: format 12 has W in {}'.format(lanes, ', '.join(str(v) for v in RANS_LANES)))
        for t, s in enumerate(streams):
            if len(s) < 4 * lanes or (len(s) - 4 * lanes) % 2:
                raise ValueError('stream of tile {} holds {} bytes: the states of its {} coders have {}, and 16-bit words follow'.format(
                    t, len(s), lanes, 4 * lanes))
    return c(*((version, ae_name, pc_name, H, W, C, h, w, L, resolution, fingerprint, th, tw, first_syms, streams, payload, crcs) +
               (() if extra is None else (extra,))))


def _parse_layered(r, ae_name, pc_name, H, W, C, h, w, strict, version=FORMAT_VERSION_LAYERED):
    """the rest of a format-6 / format-8 file after the symbol volume shape -> (LayeredContainer, layers_complete, payload complete).
    The header: every length against the bytes that remain, then its own CRC.  strict (parse_container; the CRC over the file has
    been checked): the payload length must equal what is left and every segment must match its CRC.  Not strict (parse_partial): the
    payload is what arrived of it; a segment that is not whole or fails its CRC is None."""
    L, resolution, fingerprint, th, tw, ntiles, _ = _parse_tile_extent(r, h, w)
    G, = r.unpack('<H', 'layer count')
    if not 1 <= G <= MAX_LAYERS:
        raise ValueError('layer count G = {} is outside 1 .. {}'.format(G, MAX_LAYERS))
    ends = check_layer_ends(r.unpack('<{}H'.format(G), 'layer ends'), C)
    first_syms = list(r.unpack('<{}H'.format(ntiles), 'first symbols'))
    for t, f in enumerate(first_syms):
        if f >= L:
            raise ValueError('first symbol {} of tile {} is not below L = {}'.format(f, t, L))
    table = r.take(8 * G * ntiles, 'segment table')        # against the bytes that remain, before anything of its size is built
    rows = struct.unpack('<{}I'.format(2 * G * ntiles), table)
    lengths = [[rows[2 * (g * ntiles + t)] for t in range(ntiles)] for g in range(G)]
    crcs = [[rows[2 * (g * ntiles + t) + 1] for t in range(ntiles)] for g in range(G)]
    n, = r.unpack('<Q', 'payload length')
    total = sum(sum(layer) for layer in lengths)
    if total != n:
        raise ValueError('segment lengths of the {} layers of {} tiles sum to {}, the payload length is {}'.format(G, ntiles, total, n))
    end = r.pos
    stored, = r.unpack('<I', 'header CRC')
    actual = zlib.crc32(r.data[:end]) & 0xffffffff
    if stored != actual:
        raise ValueError('header CRC mismatch: file says {:08x}, the header gives {:08x}'.format(stored, actual))
    left = len(r.data) - r.pos
    if strict and n != left:
        raise ValueError('payload length {} does not equal the {} bytes that remain in the file'.format(n, left))
    payload = r.data[r.pos:r.pos + n]
    segments, pos, complete = [], 0, 0
    for g in range(G):
        layer = []
        for t in range(ntiles):
            b = payload[pos:pos + lengths[g][t]]
            pos += lengths[g][t]
            if pos <= len(payload) and zlib.crc32(b) & 0xffffffff == crcs[g][t]:
                layer.append(b)
            elif strict:
                raise ValueError('segment CRC mismatch in layer {}, tile {}: the table says {:08x}, the segment gives {:08x}'.format(
                    g, t, crcs[g][t], zlib.crc32(b) & 0xffffffff))
            else:
                layer.append(None)
        if complete == g and all(b is not None for b in layer):
            complete = g + 1
        segments.append(layer)
    streams = [[segments[g][t] for g in range(G)] for t in range(ntiles)]
    c = LayeredContainer(version, ae_name, pc_name, H, W, C, h, w, L, resolution, fingerprint, th, tw, first_syms, streams,
                         payload, ends, segments, crcs)
    return c, complete, len(payload) == n


def _check_layer_index(g, G):
    if isinstance(g, (bool, np.bool_)) or not isinstance(g, (int, np.integer)) or not 0 <= int(g) <= G:
        raise ValueError('layer prefix: g = {!r} is outside 0 .. G = {}'.format(g, G))
    return int(g)


def layer_prefix_bytes(data_or_container, g):
    """the length of the prefix of a format-6 file that holds the header and the layers 0 .. g - 1 of every tile, g in 0 .. G
    (g = 0: the header alone; g = G: the file without its last 4 bytes, the CRC over the file).  Takes the file's bytes -- a prefix
    that holds the whole header will do -- or a LayeredContainer of parse_container."""
    c = data_or_container
    if not isinstance(c, LayeredContainer):
        return _prefix_from_bytes(bytes(c), g)
    g = _check_layer_index(g, len(c.layer_ends))
    if any(b is None for layer in c.segments[:g] for b in layer):
        raise ValueError('layer prefix: this container has incomplete layers, take the lengths from the bytes of the file')
    a, p, nt, G = len(c.ae_name.encode('utf-8')), len(c.pc_name.encode('utf-8')), len(c.first_syms), len(c.layer_ends)
    header = 4 + 2 + 2 + a + 2 + p + 8 + 10 + 2 + 8 + 4 + 4 + 4 + 2 + 2 * G + 2 * nt + 8 * G * nt + 8 + 4
    return header + sum(len(b) for layer in c.segments[:g] for b in layer)


def _prefix_from_bytes(data, g):
    r, version = _partial_open(data)
    try:
        ae_name, pc_name, H, W, C, h, w = _parse_front(r)
        L, resolution, fingerprint, th, tw, ntiles, _ = _parse_tile_extent(r, h, w)
        G, = r.unpack('<H', 'layer count')
        if not 1 <= G <= MAX_LAYERS:
            raise ValueError('layer count G = {} is outside 1 .. {}'.format(G, MAX_LAYERS))
        r.take(2 * G + 2 * ntiles, 'layer ends and first symbols')
        rows = struct.unpack('<{}I'.format(2 * G * ntiles), r.take(8 * G * ntiles, 'segment table'))
        r.take(8, 'payload length')
        end = r.pos
        stored, = r.unpack('<I', 'header CRC')
    except ValueError as e:
        raise ValueError('header damaged: {}'.format(e))
    if stored != zlib.crc32(data[:end]) & 0xffffffff:
        raise ValueError('header damaged: header CRC mismatch')
    return r.pos + sum(rows[2 * i] for i in range(_check_layer_index(g, G) * ntiles))


def _refuse(data, what):
    """--salvage, --partial, --recover, stream and repair (`what`) do not read a format that carries the checksums they read by but
    has none of them among its readers -- formats 10 and 12: one sentence, before anything else of the file is looked at.  The
    formats without checksums and each other's formats they refuse in words of their own."""
    row = FORMATS.get(_source_version(data))
    if row is not None and row.checked and not row.readers:
        raise ValueError('format version {} ({}) is not read by {}: a file to be salvaged is written with --tile --checked or --tile '
                         '--wavefront (versions {} and {}), a file to be read from a prefix, recovered or streamed with the layered '
                         'formats --layers / --front-layers (versions {} and {}); an intact file decodes with decompress'.format(
                             row.version, row.name, what, FORMAT_VERSION_CHECKED, FORMAT_VERSION_WAVEFRONT, FORMAT_VERSION_LAYERED,
                             FORMAT_VERSION_FRONTS))


def _partial_open(data):
    if len(data) < _MIN_SIZE:
        raise ValueError('header damaged: truncated file: {} bytes, the smallest container has {}'.format(len(data), _MIN_SIZE))
    if data[:4] != MAGIC:
        raise ValueError('header damaged: wrong magic {!r}: not a codec file (expected {!r})'.format(data[:4], MAGIC))
    _refuse(data, '--partial / --recover / stream')
    version, = struct.unpack('<H', data[4:6])
    if version not in _LAYERED_VERSIONS:
        raise ValueError('header damaged: format version {} is not the layered version {}: only a layered file (--tile --layers / '
                         '--progressive) decodes from a prefix'.format(version, FORMAT_VERSION_LAYERED))
    return _Reader(data), version


def parse_partial(data):
    """a prefix of a format-6 file (or the whole file, or a damaged one) -> (LayeredContainer, layers_complete, file_crc_ok).
    The header must be whole and pass its own CRC, else ValueError('header damaged: ...').  Behind it nothing raises: a layer is
    complete when all its segments are there and match their CRCs, layers_complete counts the leading complete layers, every
    segment that is not whole or fails its CRC is None in the container; file_crc_ok says whether the CRC over the file is there
    and right.  Bytes behind the declared end are ignored."""
    data = bytes(data)
    r, version = _partial_open(data)
    try:
        ae_name, pc_name, H, W, C, h, w = _parse_front(r)
        c, complete, whole = _parse_layered(r, ae_name, pc_name, H, W, C, h, w, strict=False, version=version)
    except ValueError as e:
        raise ValueError('header damaged: nothing can be decoded ({})'.format(e))
    end = _prefix_from_bytes(data, len(c.layer_ends))       # where the CRC over the file stands
    tail = data[end:end + 4]
    file_crc_ok = whole and len(tail) == 4 and struct.unpack('<I', tail)[0] == zlib.crc32(data[:end]) & 0xffffffff
    return c, complete, bool(file_crc_ok)


def parse_recover(data):
    """a format-6 file, whole, cut or damaged -> (LayeredContainer, layers, reasons, file_crc_ok).  layers[t] is the number of LEADING
    segments of tile t that are wholly there and match their CRCs, 0 .. G: an intact segment behind a bad one cannot be decoded and is
    dropped.  reasons: {tile: 'crc' | 'truncated'} for the tiles with layers[t] < G, that of the tile's first bad segment ('truncated':
    its byte range is not complete; 'crc': the bytes are there, their CRC differs).  The header must be whole and pass its own CRC, as
    for parse_partial, else ValueError('header damaged: ...'); behind it nothing raises.  Another format is a ValueError."""
    data = bytes(data)
    version = _source_version(data)
    if version in (FORMAT_VERSION, FORMAT_VERSION_TILED) + _WITH_CRCS:
        raise ValueError('format version {} is not the layered version {}: --recover reads layered files (--tile --layers / --progressive); '
                         'a damaged format-{} / format-{} file is read with --salvage, an intact file of any format with '
                         'decompress'.format(version, FORMAT_VERSION_LAYERED, FORMAT_VERSION_CHECKED, FORMAT_VERSION_WAVEFRONT))
    c, _, file_crc_ok = parse_partial(data)
    G, ntiles = len(c.layer_ends), len(c.first_syms)
    start = _prefix_from_bytes(data, 0)                    # the payload's first byte; in front of it: header CRC, payload length, table
    rows = struct.unpack_from('<{}I'.format(2 * G * ntiles), data, start - 4 - 8 - 8 * G * ntiles)
    ends, pos = [[0] * ntiles for _ in range(G)], 0       # where segment (g, t) ends in the payload
    for g in range(G):
        for t in range(ntiles):
            pos += rows[2 * (g * ntiles + t)]
            ends[g][t] = pos
    layers, reasons = [], {}
    for t in range(ntiles):
        g_t = 0
        while g_t < G and c.segments[g_t][t] is not None:
            g_t += 1
        layers.append(g_t)
        if g_t < G:
            reasons[t] = 'truncated' if ends[g_t][t] > len(c.payload) else 'crc'
    return c, layers, reasons, file_crc_ok


def resume_plan(done_layers, now_layers, layer_ends):
    """what a decoder that holds the leading `done_layers` layers of a tile has to do when `now_layers` of them are there ->
    (from_layer, channels) as ic_pc_decode_tiles_batch_layers_resume_f32 takes them per tile: continue with layer from_layer up to
    channel `channels`.  done <= now: (done, e_{now-1}) -- with done == now nothing is decoded, the call only rewrites the fill above
    the limit, and done == now == G says the tile is whole.  done == 0 (nothing yet, or a decoder failure dropped what there was):
    the fresh start (0, e_{now-1}).  now < done (the caller takes layers back): a fresh start as well, what is held above is of no
    use.  now == 0: (0, 0), the tile stays out of the launch."""
    G = len(layer_ends)
    done, now = int(done_layers), int(now_layers)
    if not 0 <= done <= G or not 0 <= now <= G:
        raise ValueError('resume plan: {} layers done, {} there now, of G = {}'.format(done, now, G))
    if now == 0:
        return 0, 0
    return (done if done <= now else 0), int(layer_ends[now - 1])


def stream_header_bytes(data, fronts=False):
    """the length of the header of the format-6 file (fronts=True: format-6 or format-8 file, which share the layout) that begins with
    `data` (magic up to and including the header CRC), or None
    while `data` is too short to tell.  A ValueError as soon as the bytes cannot be the beginning of a format-6 file: wrong magic,
    another format (parse_recover's words), a layer count or a tile count that does not fit the rest.  Nothing is checked that the
    whole header's own CRC covers: parse_recover does that once the header is there."""
    data = bytes(data)
    if data[:4] != MAGIC[:len(data[:4])]:
        raise ValueError('header damaged: wrong magic {!r}: not a codec file (expected {!r})'.format(data[:4], MAGIC))
    if len(data) < 6:
        return None
    version, = struct.unpack('<H', data[4:6])
    if version == FORMAT_VERSION_FRONTS and not fronts:
        raise ValueError('format version {} (front-layered tiles) is not streamed without --fronts (open_stream(fronts=True)), which '
                         'continues a front-ordered decode; decompress --recover (Codec.recover) also reads what has arrived of such '
                         'a file'.format(version))
    if version != FORMAT_VERSION_LAYERED and not (fronts and version == FORMAT_VERSION_FRONTS):
        parse_recover(data + bytes(_MIN_SIZE))            # another format: its refusal, whatever the length so far
        raise ValueError('header damaged: format version {} is not the layered version {}'.format(version, FORMAT_VERSION_LAYERED))
    if len(data) < 8:
        return None
    a, = struct.unpack('<H', data[6:8])
    if len(data) < 10 + a:
        return None
    p, = struct.unpack('<H', data[8 + a:10 + a])
    base = 10 + a + p                                      # H, W, C, h, w, L, resolution, fingerprint, th, tw, ntiles, G: 42 bytes
    if len(data) < base + 42:
        return None
    h, w = struct.unpack('<II', data[base + 10:base + 18])
    th, tw, nt, G = struct.unpack('<HHIH', data[base + 32:base + 42])
    if not 1 <= G <= MAX_LAYERS:
        raise ValueError('header damaged: layer count G = {} is outside 1 .. {}'.format(G, MAX_LAYERS))
    if th < 1 or tw < 1 or h < 1 or w < 1 or nt != ((h + th - 1) // th) * ((w + tw - 1) // tw):
        raise ValueError('header damaged: {} tiles do not cover a {} x {} volume with tiles of {} x {}'.format(nt, h, w, th, tw))
    return base + 42 + 2 * G + 2 * nt + 8 * G * nt + 8 + 4


def parse_salvage(data):
    """what a possibly damaged format-4 or format-5 file still holds -> (CheckedContainer or WavefrontContainer, damage, file_crc_ok).  damage: [(tile, reason)] in
    tile order, reason 'crc' (the bytes are there, their CRC differs) or 'truncated' (the tile's byte range is not complete);
    streams[t] of such a tile is None.  Order: size, magic, version, then the header up to its own CRC, every length against the
    bytes that are there; a header that fails its CRC is a ValueError, nothing of it is believed.  Behind a good header the
    payload is what follows, at most the declared n bytes; the CRC over the file is not required, file_crc_ok says whether it is
    there and right; bytes behind the declared end are ignored."""
    data = bytes(data)
    if len(data) < _MIN_SIZE:
        raise ValueError('truncated file: {} bytes, the smallest container has {}'.format(len(data), _MIN_SIZE))
    if data[:4] != MAGIC:
        raise ValueError('wrong magic {!r}: not a codec file (expected {!r})'.format(data[:4], MAGIC))
    version, = struct.unpack('<H', data[4:6])
    _refuse(data, '--salvage')
    if version in (FORMAT_VERSION, FORMAT_VERSION_TILED):
        raise ValueError('format version {} has nothing to salvage with: one CRC over the whole file, none per tile (only version {}, '
                         'written with --tile --checked, can be salvaged)'.format(version, FORMAT_VERSION_CHECKED))
    if version in _LAYERED_VERSIONS:
        raise ValueError('format version {} (layered tiles) is not salvaged: salvage of layered files is out of scope; '
                         'decompress --partial (Codec.decompress_partial) reads the complete layers of a cut file'.format(version))
    if version not in _WITH_CRCS:
        raise ValueError('unsupported format version {} (only version {} can be salvaged) or the wavefront version {}'.format(
            version, FORMAT_VERSION_CHECKED, FORMAT_VERSION_WAVEFRONT))
    r = _Reader(data)
    try:
        ae_name, pc_name, H, W, C, h, w = _parse_front(r)
        L, resolution, fingerprint, th, tw, first_syms, lengths, crcs, n, _ = _parse_tile_table(r, version, h, w)
        end = r.pos
        stored, = r.unpack('<I', 'header CRC')
    except ValueError as e:
        # the header's own words cannot be told from damage before its CRC has been seen
        raise ValueError('header damaged: nothing can be recovered ({})'.format(e))
    actual = zlib.crc32(data[:end]) & 0xffffffff
    if stored != actual:
        raise ValueError('header damaged: nothing can be recovered (header CRC mismatch: file says {:08x}, the header of this '
                         'version-{} file gives {:08x})'.format(stored, version, actual))
    start = r.pos
    payload = data[start:start + n]                        # what arrived of it
    streams, damage, pos = [], [], 0
    for t, (n_t, crc) in enumerate(zip(lengths, crcs)):
        if n_t and pos + n_t > len(payload):           # (an empty stream is complete wherever the file ends)
            streams.append(None)
            damage.append((t, 'truncated'))
        elif zlib.crc32(payload[pos:pos + n_t]) & 0xffffffff != crc:
            streams.append(None)
            damage.append((t, 'crc'))
        else:
            streams.append(payload[pos:pos + n_t])
        pos += n_t
    tail = data[start + n:start + n + 4]
    file_crc_ok = len(payload) == n and len(tail) == 4 and struct.unpack('<I', tail)[0] == zlib.crc32(data[:start + n]) & 0xffffffff
    c = FORMATS[version].container(version, ae_name, pc_name, H, W, C, h, w, L, resolution, fingerprint, th, tw, first_syms, streams, payload, crcs)
    return c, damage, file_crc_ok


def model_fingerprint(centers, pc_params):
    """CRC-32 over the float32 little-endian bytes of the centres, then of the context model's variables in the order of their
    names (sorted): the tables of the range coder are a function of exactly these."""
    crc = zlib.crc32(np.ascontiguousarray(np.asarray(centers), dtype='<f4').tobytes())
    for name in sorted(pc_params):
        crc = zlib.crc32(name.encode('utf-8'), crc)
        crc = zlib.crc32(np.ascontiguousarray(np.asarray(pc_params[name]), dtype='<f4').tobytes(), crc)
    return crc & 0xffffffff


def config_name(config):
    """'cvpr/low' for .../ae_configs/cvpr/low: the path below the config tree, else the file name."""
    parts = os.path.normpath(str(config._path)).split(os.sep)
    for i, comp in enumerate(parts):
        if comp in ('ae_configs', 'pc_configs') and i + 1 < len(parts):
            return '/'.join(parts[i + 1:])
    return parts[-1]


class Codec(object):
    """builds the networks once (as val.Fetcher does); compress / decompress map HWC uint8 images to container bytes and back.
    device_encode: which range encoder writes the payload -- the bytes are the same either way (tests/test_gpu_codec.py); the
    default is the one that measured faster end to end on a Kodak volume.
    tile: None writes format 1; (th, tw) in symbol-volume units writes format 2, one stream per tile; with checked=True format 4,
    the same streams with a CRC each (salvage reads what a damaged one still holds).  order: 'raster' as above; 'wavefront' (needs
    a tile extent) writes format 5, the layout of format 4 with every tile's symbols coded front by front, which the decoder
    takes a front at a time -- refused here, with a ValueError, for a context model whose masks do not make T = x + 2 y + 4 c a
    valid order or whose width the wavefront decoder does not cover.  layers: None as above; 'default' (default_layer_ends(C)) or a
    sequence of layer ends e_0 < .. < e_{G-1} = C writes format 6, every tile's raster stream cut into G segments and stored layer
    first, so that a prefix of the file decodes (decompress_partial); needs a tile extent, not with order='wavefront', carries the
    checksums whatever `checked` says; refused, like the wavefront order, for a context model of another width than k = 24.
    front_layers: None as above; 'default' or a sequence of layer ends writes format 8, the layout of format 6 with every tile's
    WAVEFRONT-ordered stream cut at fronts (front_layer_cuts): decoded a front at a time like format 5, read from a prefix like
    format 6.  Needs a tile extent; not with layers or order='wavefront' (it is neither format 6 nor format 5: the order is implied);
    refused for a model that either of those refuses.
    Reading needs no option: the file's version decides."""

    def __init__(self, ae_config, pc_config, weights, device='cuda', plan_flags=0, device_encode=True, tile=None, checked=False,
                 order='raster', layers=None, front_layers=None, depth_block=None, rans=None):
        if tile is not None:
            tile = (int(tile[0]), int(tile[1]))
            if not (1 <= tile[0] <= 0xffff and 1 <= tile[1] <= 0xffff):
                raise ValueError('tile extent {} x {} is outside 1 .. 65535'.format(*tile))
        self.tile, self.checked, self.order, self.layers, self.front_layers = tile, bool(checked), order, layers, front_layers
        self.depth_block, self.rans = depth_block, rans
        self.C = getattr(ae_config, 'num_chan_bn', None)
        self.wavefront_refusal = self.layered_refusal = self.depth_refusal = self.rans_refusal = self.rdo_refusal = None
        self._target()                                               # the combinations: refused before any model is built
        import torch
        from . import autoencoder, probclass
        self.device = torch.device(device)
        self.ae = autoencoder.get_network_cls(ae_config)(ae_config).load_weights(weights, self.device)
        self.pc = probclass.get_network_cls(pc_config)(pc_config, num_centers=ae_config.num_centers).load_weights(weights, self.device)
        self.ae.plan_flags = int(plan_flags)
        try:
            wavefront_coeffs(self.pc)
            self.wavefront_refusal = None
        except ValueError as e:
            self.wavefront_refusal = str(e)
        k = int(getattr(self.pc, '_k', None) or pc_config.arch_param__k)
        self.layered_refusal = None if k == 24 else ('layered tiles: the decoder that restarts at layer cuts covers context models of '
                                                     'width k = 24, this one has k = {}'.format(k))
        self.depth_refusal = self.wavefront_refusal or (None if k == 24 else (
            'depth-mapped tiles: the front decoder that reads a depth plane covers context models of width k = 24, this one has '
            'k = {}'.format(k)))
        self.rans_refusal = self.wavefront_refusal or (None if k == 24 else (
            'lane-parallel rANS tiles: the front decoder that steps W coders at once covers context models of width k = 24, this one '
            'has k = {}'.format(k)))
        self.rdo_refusal = ('rate-aware symbol choice: the front sweep that chooses symbols covers context models of width k = 24, this '
                            'one has k = {}'.format(k)) if k != 24 else self.wavefront_refusal      # (no format's: raised only when rdo is asked for)
        self._target()                                               # the model's refusal of the format asked for
        self.pred =probclass.PredictionNetwork(self.pc, pc_config, self.ae.get_centers_variable())
        self.ae_name, self.pc_name = config_name(ae_config), config_name(pc_config)
        self.factor = int(self.ae.get_subsampling_factor())
        self.C, self.L = int(ae_config.num_chan_bn), int(ae_config.num_centers)
        self.device_encode = bool(device_encode)
        self.fingerprint = model_fingerprint(self.ae.get_centers_variable().detach().cpu().numpy(),
                                             {n: t.detach().cpu().numpy() for n, t in self.pc._params.items()})

    # -- the two halves, also usable on their own (tests compare their intermediate values) --

    def encode_symbols(self, img_hwc_uint8):
        """HWC uint8 -> (EncoderOutput of the padded image, (H, W))."""
        x, size = self._image_tensor(img_hwc_uint8)
        return self.ae.encode(x, is_training=False), size

    def _host_encode_stream(self, symbols_chw):
        """the parent path: all tables to the host, the Python coder over them.  Same bytes as encode_stream."""
        from . import arithmetic_coding as ac

        class _Keep(io.BytesIO):
            def close(self):            # encode_sequence closes its file object: keep the bytes
                self.kept = self.getvalue()
                io.BytesIO.close(self)

        _, freqs = self.pred.get_all(self.pred.pad_symbols_volume(symbols_chw))
        flat = symbols_chw.reshape(-1).astype(np.int64)
        out = _Keep()
        ac.encode_sequence(flat[1:], freqs[1:], out)
        return out.kept, int(flat[0])

    @staticmethod
    def _check_front_layers(front_layers, tile, order, layers):
        if tile is None:
            raise ValueError('front_layers needs a tile extent: format 8 is a tiled format')
        if layers is not None:
            raise ValueError('front_layers does not go with layers: the one cuts the wavefront order at fronts (format 8), the other the '
                             'raster order at channel planes (format 6)')
        if order == 'wavefront':
            raise ValueError("front_layers does not go with order='wavefront': format 8 implies the order, order='wavefront' writes the "
                             "unlayered format 5")
        if isinstance(front_layers, str) and front_layers != 'default':
            raise ValueError("front_layers is None, 'default' or a sequence of layer ends, got {!r}".format(front_layers))

    @staticmethod
    def _check_depth(depth_block, tile, order, layers, front_layers, C):
        if tile is None:
            raise ValueError('depth_block needs a tile extent: format 10 is a tiled format')
        if order == 'wavefront':
            raise ValueError("depth_block does not go with order='wavefront': format 10 implies the order, order='wavefront' writes "
                             "format 5, which codes every position")
        if layers is not None or front_layers is not None:
            raise ValueError('depth_block does not go with layers or front_layers: format 10 is one coder run per tile, the layered '
                             'formats 6 and 8 cut a tile into several')
        check_depth_block(depth_block, C)

    @staticmethod
    def _check_rans(rans, tile, checked, order, layers, front_layers, depth_block):
        if tile is None:
            raise ValueError('rans needs a tile extent: format 12 is a tiled format')
        if checked:
            raise ValueError('rans does not go with checked=True: format 12 has its own CRC per tile, checked=True writes format 4')
        if order == 'wavefront':
            raise ValueError("rans does not go with order='wavefront': format 12 implies the order, order='wavefront' writes format 5, "
                             "one arithmetic coder per tile")
        if depth_block is not None:
            raise ValueError('rans does not go with depth_block: format 10 leaves positions out of an arithmetic coder\'s stream, '
                             'format 12 codes every position with W rANS coders')
        if layers is not None or front_layers is not None:
            raise ValueError('rans does not go with layers or front_layers: format 12 is one interleaved stream per tile, the layered '
                             'formats 6 and 8 cut a tile into several')
        if not (isinstance(rans, str) and rans == 'default'):
            check_rans_lanes(rans)

    def _target(self):
        """the format this Codec writes -> (its row of FORMATS, the format's parameter: the coders W, the depth block B, the layer
        ends, or None).  Resolved on every call from the attributes as they are now -- main and the timing tools set them after
        construction -- with every refusal of a combination and of the model, in one order: rans, depth_block, front_layers, layers,
        order, checked."""
        tile, order, layers = self.tile, self.order, self.layers
        checked, fronts = getattr(self, 'checked', False), getattr(self, 'front_layers', None)
        depth, rans = getattr(self, 'depth_block', None), getattr(self, 'rans', None)
        version, param = None, None                                  # (the checks leave at most one of the four options standing)

        def allowed(refusal):
            if refusal:
                raise ValueError(refusal)

        if rans is not None:
            self._check_rans(rans, tile, checked, order, layers, fronts, depth)
            allowed(self.rans_refusal)
            version, param = FORMAT_VERSION_RANS, DEFAULT_RANS_LANES if isinstance(rans, str) else int(rans)
        if depth is not None:
            self._check_depth(depth, tile, order, layers, fronts, self.C)
            allowed(self.depth_refusal)
            version, param = FORMAT_VERSION_DEPTH, int(depth)
        if fronts is not None:
            self._check_front_layers(fronts, tile, order, layers)
            allowed(self.wavefront_refusal or self.layered_refusal)
            version, param = FORMAT_VERSION_FRONTS, default_layer_ends(self.C) if isinstance(fronts, str) else check_layer_ends(fronts, self.C)
        if layers is not None:
            if tile is None:
                raise ValueError('layers needs a tile extent: format 6 is a tiled format')
            if order == 'wavefront':
                raise ValueError("layers does not go with order='wavefront': a layer is no prefix of a wavefront-ordered stream")
            allowed(self.layered_refusal)
            if isinstance(layers, str) and layers != 'default':
                raise ValueError("layers is None, 'default' or a sequence of layer ends, got {!r}".format(layers))
            version, param = FORMAT_VERSION_LAYERED, default_layer_ends(self.C) if isinstance(layers, str) else check_layer_ends(layers, self.C)
        if order not in ('raster', 'wavefront'):
            raise ValueError("order is 'raster' or 'wavefront', got {!r}".format(order))
        if order == 'wavefront':
            if tile is None:
                raise ValueError("order='wavefront' needs a tile extent: format 5 is a tiled format")
            allowed(self.wavefront_refusal)
            version = FORMAT_VERSION_WAVEFRONT                       # (checked or not: format 5 always carries the checksums)
        if checked and tile is None:
            raise ValueError('checked=True needs a tile extent: the checksums of format 4 are per tile')
        if version is None:
            version = FORMAT_VERSION if tile is None else FORMAT_VERSION_CHECKED if checked else FORMAT_VERSION_TILED
        return FORMATS[version], param

    def _front_ends(self):
        """the layer ends of the format-8 file compress writes, or None"""
        row, param = self._target()
        return param if row.version == FORMAT_VERSION_FRONTS else None

    def compress(self, img_hwc_uint8, cap=None, rois=None, background=None, rdo=None):
        """HWC uint8 -> container bytes.  cap: None, a level, or an (h, w) plane bounding the importance map (cap_plane; rois and
        background as there, the level inside the rectangles); without any of them the encoder's own operating point.
        rdo: None, or lambda >= 0 -- a number, or one per tile of this Codec's grid in tile_grid order (format 1: one): the symbols
        are those of choose_symbols, chosen by distortion + lambda * rate under the context model, in place of the quantiser's;
        the file's format and every reader are what they are without it, and rdo=0 is the file of rdo=None byte for byte."""
        if rdo is not None:
            sym, _, (H, W) = self.choose_symbols(img_hwc_uint8, rdo, cap=cap, rois=rois, background=background)
            return self._container(sym, H, W)
        if cap is None and not rois and background is None:
            enc, (H, W) = self.encode_symbols(img_hwc_uint8)
        else:
            enc, _, (H, W) = self.encode_symbols_capped(img_hwc_uint8, cap, rois, background)
        return self._container(enc.symbols[0], H, W)

    def _rdo_tile(self, h, w):
        """the coded volumes a sweep runs over: this Codec's tiles, or the whole (h, w) volume for format 1"""
        return self.tile if self.tile is not None else (int(h), int(w))

    def choose_symbols(self, img_hwc_uint8, rdo, cap=None, rois=None, background=None):
        """compress's symbols under rdo -> ((C, h, w) int64 device tensor, EncoderOutput, (H, W)).  z is the masked bottleneck of
        the encoder pass that compress runs, capped or not; every tile of this Codec's grid (the whole volume for format 1) is
        swept front by front, each position taking the first symbol that attains min_j k_j + Lambda R_j (rdo_choose) given the
        symbols already chosen (PredictionNetwork.choose_tiles_batch).  A ValueError (rdo_refusal) for a context model of another
        width than k = 24."""
        if self.rdo_refusal:
            raise ValueError(self.rdo_refusal)
        self._target()
        if cap is None and not rois and background is None:
            enc, (H, W) = self.encode_symbols(img_hwc_uint8)
        else:
            enc, _, (H, W) = self.encode_symbols_capped(img_hwc_uint8, cap, rois, background)
        z = enc.z[0].contiguous()
        th, tw = self._rdo_tile(z.shape[1], z.shape[2])
        return self.pred.choose_tiles_batch([z], th, tw, [rdo])[0], enc, (H, W)

    def _image_tensor(self, img_hwc_uint8, what=''):
        """HWC uint8 -> ((1, 3, H', W') float32 device tensor of the padded image, (H, W))"""
        import torch
        from . import val
        img = np.asarray(img_hwc_uint8)
        if img.ndim != 3 or img.shape[2] not in (3, 4) or img.dtype != np.uint8:
            raise ValueError('{}expected an HWC uint8 image with 3 channels, got {} {}'.format(what, img.shape, img.dtype))
        img = img[:, :, :3]
        padded, _ = val.add_padding(img, self.factor)
        x = torch.as_tensor(np.ascontiguousarray(np.transpose(padded, (2, 0, 1)))[None]).to(self.device).float()
        return x, (int(img.shape[0]), int(img.shape[1]))

    def cap_plane(self, H, W, cap=None, rois=None, background=None):
        """compress's cap argument for an H x W image -> the (h, w) float32 plane: a plane is checked, a level goes through cap_plane"""
        if cap is not None and np.ndim(cap) > 0:
            f = self.factor
            plane = np.asarray(cap)
            if plane.shape != ((H + f - 1) // f, (W + f - 1) // f):
                raise ValueError('cap plane of shape {} for a {} x {} image: expected {}'.format(plane.shape, H, W, ((H + f - 1) // f, (W + f - 1) // f)))
            if rois or background is not None:
                raise ValueError('rois / background do not go with a cap plane: they are a way of making one (cap_plane)')
            plane = plane.astype(np.float32)
            if not bool((plane >= 0).all()):
                raise ValueError('cap plane: entries must be in [0, +inf], got a negative or NaN entry')
            return np.ascontiguousarray(plane)
        return cap_plane(H, W, self.factor, level=cap, rois=rois or (), background=background)

    def encode_symbols_capped(self, img_hwc_uint8, cap=None, rois=None, background=None, keep_bottleneck=False):
        """encode_symbols under a cap (compress's arguments) -> (EncoderOutput, bottleneck or None, (H, W))"""
        import torch
        x, (H, W) = self._image_tensor(img_hwc_uint8)
        plane = torch.as_tensor(self.cap_plane(H, W, cap, rois, background)[None]).to(self.device)
        enc, bott = self.ae.encode_capped(x, plane, keep_bottleneck=keep_bottleneck)
        return enc, bott, (H, W)

    def compress_to_budget(self, img_hwc_uint8, max_bytes, rois=None):
        """the largest level of cap_levels(C) whose file has at most max_bytes bytes -> (data, level, probes): data is byte for byte
        compress(img, cap=level), or with rois compress(img, rois=rois, background=level) (the rectangles stay uncapped, the budget
        is met by the background); probes is the number of real codings.  The encoder runs once; every level after that is a
        requantisation of its bottleneck.  An estimate from the context model's bit costs (up to 16 levels a launch, one
        readback a round) starts budget_search, whose contract holds on the real files: data fits, and the next level's file
        does not (or level == C).  A ValueError if the file of level 0 is over the budget."""
        import torch
        from ._lib import lib, check, ptr, current_stream
        max_bytes = int(max_bytes)
        x, (H, W) = self._image_tensor(img_hwc_uint8)
        _, bott = self.ae.encode_capped(x, None, keep_bottleneck=True)
        levels = cap_levels(self.C)
        h, w = int(bott.shape[2]), int(bott.shape[3])
        roi = torch.as_tensor(np.isinf(cap_plane(H, W, self.factor, rois=rois, background=0.0))).to(self.device) if rois else None
        lv = torch.as_tensor(levels).to(self.device)
        inf = torch.full((), float('inf'), dtype=torch.float32, device=self.device)

        def planes(ks):                                               # (1, T, h, w): level k outside the rectangles, +inf inside
            p = lv[torch.as_tensor(list(ks), device=self.device)][:, None, None].expand(len(ks), h, w)
            return (p if roi is None else torch.where(roi[None], inf, p))[None].contiguous()

        files = {}

        def coded(k):
            if k not in files:
                files[k] = self._container(self.ae.requantize(bott, planes([k]), hard_only=True).symbols[0], H, W)
            return files[k]

        def estimate(ks):                                             # bytes of the whole-volume pass per level, one readback
            enc = self.ae.requantize(bott, planes(ks), hard_only=True)
            bits = self.pc.bitcost(enc.qhard, enc.symbols, is_training=False, pad_value=self.pc.auto_pad_value(self.ae))
            buf = torch.empty(1024 + len(ks), dtype=torch.float32, device=self.device)
            check(lib.ic_mean_rows_f32(ptr(bits), len(ks), bits.numel() // len(ks), 8.0, ptr(buf), ptr(buf[1024:]),
                                       current_stream(self.device)), 'ic_mean_rows_f32')
            return [float(v) for v in buf[1024:].cpu().numpy()]

        guess = CAP_STEPS
        if len(coded(CAP_STEPS)) > max_bytes:
            # the container and the streams' ends cost the same at every level, to first order: take them from the one real file
            ks = list(range(16, CAP_STEPS + 1, 16))
            est = estimate(ks)
            room = max_bytes - (len(files[CAP_STEPS]) - est[-1])
            below = [k for k, b in zip(ks, est) if b <= room]
            ks = list(range(1, 16)) if not below else list(range(below[-1] + 1, min(below[-1] + 16, CAP_STEPS)))
            guess = below[-1] if below else 0
            if ks:
                fit = [k for k, b in zip(ks, estimate(ks)) if b <= room]
                guess = fit[-1] if fit else guess
        try:
            k, probes = budget_search(lambda k: len(coded(k)) <= max_bytes, guess)
        except ValueError:
            raise ValueError('budget of {} bytes: the smallest file, at level 0, has {} bytes'.format(max_bytes, len(coded(0))))
        return files[k], float(levels[k]), probes

    def _container(self, sym, H, W):
        """the symbols (C, h, w) of an H x W image, on the device -> container bytes in this Codec's format"""
        row, param = self._target()
        if row.version != FORMAT_VERSION:
            return self._pack(row, param, self.pred.encode_tiles(sym, self.tile[0], self.tile[1], **_coder_kw(row, param)), sym, H, W)
        C, h, w = (int(v) for v in sym.shape)
        if self.device_encode:
            payload, first_sym = self.pred.encode_stream(sym)
        else:
            payload, first_sym = self._host_encode_stream(sym.cpu().numpy())
        return build_container(self.ae_name, self.pc_name, H, W, C, h, w, self.L, first_sym, self.pred.freqs_resolution,
                               self.fingerprint, payload)

    def _pack(self, row, param, coded, sym, H, W):
        """the coded tiles of one volume, as encode_tiles gives them for the tiled format `row` -> its container bytes"""
        C, h, w = (int(v) for v in sym.shape)
        head = (self.ae_name, self.pc_name, H, W, C, h, w, self.L, self.pred.freqs_resolution, self.fingerprint) + tuple(self.tile)
        if row.layered:
            return build_layered_container(*(head + ([f for _, f in coded], param, [[segs[g] for segs, _ in coded] for g in range(len(param))])),
                                           version=row.version)
        return _build_tiled(row.version, *(head + ([f for _, f in coded], [b for b, _ in coded], param)))

    def check_container(self, c):
        """the header against the loaded model and against itself; the volume is bounded by the header's own image size only (a
        confident table codes a symbol in far less than a bit: the payload length says nothing about the symbol count)."""
        if (c.ae_name, c.pc_name) != (self.ae_name, self.pc_name):
            raise ValueError('config mismatch: the file was written with {} / {}, the loaded model is {} / {}'.format(
                c.ae_name, c.pc_name, self.ae_name, self.pc_name))
        if c.fingerprint != self.fingerprint:
            raise ValueError('model fingerprint mismatch: the file was written by model {:08x}, the loaded model is {:08x} '
                             '(other weights would decode other symbols)'.format(c.fingerprint, self.fingerprint))
        if c.C != self.C or c.L != self.L:
            raise ValueError('header mismatch: C = {}, L = {} in the file, the model has C = {}, L = {}'.format(c.C, c.L, self.C, self.L))
        if c.H < 1 or c.W < 1:
            raise ValueError('header mismatch: image size {} x {}'.format(c.H, c.W))
        f = self.factor
        eh, ew = (c.H + f - 1) // f, (c.W + f - 1) // f
        if (c.h, c.w) != (eh, ew):
            raise ValueError('header mismatch: symbol volume {} x {} does not belong to a {} x {} image (expected {} x {})'.format(
                c.h, c.w, c.H, c.W, eh, ew))
        for refusal in FORMATS[c.version].refusals:
            if getattr(self, refusal):
                raise ValueError('format {} cannot be read with this model: {}'.format(c.version, getattr(self, refusal)))
        for first_sym in (c.first_syms if isinstance(c, _TILED) else [c.first_sym]):
            if first_sym >= c.L:
                raise ValueError('header mismatch: first symbol {} is not below L = {}'.format(first_sym, c.L))
        if c.resolution != self.pred.freqs_resolution:
            raise ValueError('header mismatch: frequency resolution {} in the file, {} in the model'.format(
                c.resolution, self.pred.freqs_resolution))

    def decode_symbols(self, data, channels=None):
        """container bytes of either format -> (symbols (C,h,w) int64 numpy, Container or TiledContainer).
        channels=K: a preview -- only channels 0 .. K - 1 are decoded, the result is preview_symbols(full decode, K, fill symbol)."""
        channels = check_channels(channels, self.C)
        c = parse_container(data)
        self.check_container(c)
        try:
            if not isinstance(c, _TILED):
                sym = self.pred.decode_stream(c.payload, (c.C, c.h, c.w), c.first_sym, channels=channels)
            elif FORMATS[c.version].order == 'raster':   # formats 2 and 4: the entry of one volume
                sym = self.pred.decode_tiles(c.streams, c.first_syms, (c.C, c.h, c.w), c.th, c.tw, channels=channels)
            else:                                        # a batch of one: the order, the ends and the extra field are arguments of the batch entry
                sym = self.pred.decode_tiles_batch([(c.streams, c.first_syms, (c.C, c.h, c.w))], c.th, c.tw, want='symbols',
                                                   channels=channels, **_decode_kw(c))[0].cpu().numpy()
        except ValueError as e:
            raise ValueError('decoder status is not 0: {}'.format(e))
        return sym, c

    def decompress_partial(self, data):
        """a prefix of a format-6 file -> (HWC uint8 image, PartialReport(layers_total, layers_decoded, channels, file_crc_ok)): the
        leading complete layers (parse_partial) decoded as the preview of their channels, decompress(whole file, channels=e_{g-1});
        the whole file gives decompress(data).  A ValueError for another format, a damaged header, another model, no complete layer."""
        c, complete, file_crc_ok = parse_partial(data)
        self.check_container(c)
        if complete < 1:
            raise ValueError('no complete layer: the file holds {} bytes, layer 0 ends at byte {}'.format(len(data), layer_prefix_bytes(data, 1)))
        channels = c.layer_ends[complete - 1]
        try:
            sym = self.pred.decode_tiles_batch([(c.streams, c.first_syms, (c.C, c.h, c.w))], c.th, c.tw, want='symbols',
                                               channels=channels, **_decode_kw(c))[0].cpu().numpy()
        except ValueError as e:
            raise ValueError('decoder status is not 0: {}'.format(e))
        return self._image(sym, c), PartialReport(len(c.layer_ends), complete, channels, file_crc_ok)

    def decompress(self, data, channels=None):
        """container bytes -> HWC uint8 image; channels=K: the preview from the first K latent channels (decode_symbols)"""
        sym, c = self.decode_symbols(data, channels=channels)
        return self._image(sym, c)

    def _image(self, sym, c):
        """symbols (C,h,w) numpy of container c -> the HWC uint8 image"""
        return np.ascontiguousarray(np.transpose(self._picture(sym, c.H, c.W).cpu().numpy(), (1, 2, 0)))

    def _picture(self, sym, H, W, ae=None):
        """symbols (C,h,w), numpy or on the device, of an H x W image -> its (3, H, W) uint8 picture, left on the device: _image
        before the copy to the host.  ae: the autoencoder object that runs the pass (a lane of _in_flight; None: this Codec's own)"""
        import torch
        s = torch.as_tensor(sym).to(self.device)
        q = self.ae.get_centers_variable()[s][None].contiguous()
        x_out = (ae or self.ae).decode(q, is_training=False).to(torch.uint8)    # tf.cast truncates (val.py)
        f = self.factor
        t, l = ((-H) % f) // 2, ((-W) % f) // 2                                   # val.add_padding's offsets
        return x_out[0, :, t:t + H, l:l + W]

    # -- a list of images per call: the same bytes / pixels as the calls above, file by file --

    IN_FLIGHT = 4

    def _lanes(self, n):
        """up to IN_FLIGHT (stream, autoencoder) pairs: objects over the SAME device weights with their own workspaces
        (sharing_weights, as val.validate keeps its fetchers), so that independent batch-1 passes overlap on the device."""
        import torch
        lanes = getattr(self, '_lane_cache', None)
        if lanes is None:
            lanes = self._lane_cache = []
        while len(lanes) < min(max(int(n), 1), self.IN_FLIGHT):
            ae = self.ae.sharing_weights()
            ae.plan_flags = self.ae.plan_flags
            lanes.append((torch.cuda.Stream(device=self.device), ae))
        return lanes[:min(max(int(n), 1), self.IN_FLIGHT)]

    def _in_flight(self, items, fn):
        """fn(ae, item) -> device tensor for every item, item i on lane i % IN_FLIGHT; the current stream waits for all lanes."""
        import torch
        cur = torch.cuda.current_stream(self.device)
        lanes = self._lanes(len(items))
        for st, _ in lanes:
            st.wait_stream(cur)
        outs = []
        for i, item in enumerate(items):
            st, ae = lanes[i % len(lanes)]
            with torch.cuda.stream(st):
                out = fn(ae, item)
            out.record_stream(cur)                        # allocated on the lane's stream, consumed on the caller's
            outs.append(out)
        for st, _ in lanes:
            cur.wait_stream(st)
        return outs

    def compress_many(self, images, caps=None, rdos=None):
        """[HWC uint8] of any mix of shapes -> [container bytes], element i byte for byte compress(images[i]).  Every image goes
        through the encoder on its own (batch 1, the plan flags of compress: the kernel form of a layer depends on the batch size,
        the bytes must not), up to IN_FLIGHT at a time; then the tiles of all images are coded by one launch per tile shape.
        caps: None, or one entry per image -- None, a level or a plane, as compress's cap: element i is compress(images[i], cap=caps[i]).
        rdos: None, or one entry per image -- None, a lambda or one per tile, as compress's rdo: element i is
        compress(images[i], cap=caps[i], rdo=rdos[i]); the images that have one are swept by one chooser launch per chunk."""
        import torch
        images = list(images)
        caps = [None] * len(images) if caps is None else list(caps)
        if len(caps) != len(images):
            raise ValueError('caps: {} entries for {} images'.format(len(caps), len(images)))
        rdos = [None] * len(images) if rdos is None else list(rdos)
        if len(rdos) != len(images):
            raise ValueError('rdos: {} entries for {} images'.format(len(rdos), len(images)))
        if any(r is not None for r in rdos) and self.rdo_refusal:
            raise ValueError(self.rdo_refusal)
        if not self.device_encode:
            return [self.compress(img, cap=cap, rdo=rdo) for img, cap, rdo in zip(images, caps, rdos)]
        xs, sizes = [], []
        for i, (img, cap) in enumerate(zip(images, caps)):
            x, size = self._image_tensor(img, 'image {}: '.format(i))
            sizes.append(size)
            xs.append((x, None if cap is None else torch.as_tensor(self.cap_plane(size[0], size[1], cap)[None]).to(self.device)))
        chosen = [i for i, r in enumerate(rdos) if r is not None]
        if chosen:
            # an image with a lambda hands its z over in place of the quantiser's symbols: the sweep gives it its symbols
            def half(ae, item):
                (x, plane), rdo = item
                enc = ae.encode(x, is_training=False) if plane is None else ae.encode_capped(x, plane)[0]
                return enc.symbols[0] if rdo is None else enc.z[0].contiguous()
            syms = self._in_flight(list(zip(xs, rdos)), half)
            by_tile = {}
            for i in chosen:                                          # format 1: a sweep's tile is the volume, one launch per shape
                by_tile.setdefault(self._rdo_tile(syms[i].shape[1], syms[i].shape[2]), []).append(i)
            for (th, tw), members in by_tile.items():
                picked = self.pred.choose_tiles_batch([syms[i] for i in members], th, tw, [rdos[i] for i in members])
                for i, sym in zip(members, picked):
                    syms[i] = sym
            return self._containers(syms, sizes)
        syms = self._in_flight(xs, lambda ae, xc: (ae.encode(xc[0], is_training=False) if xc[1] is None else
                                                   ae.encode_capped(xc[0], xc[1])[0]).symbols[0])
        return self._containers(syms, sizes)

    def _containers(self, syms, sizes):
        """[(C, h, w) device symbols], [(H, W)] -> [container bytes], element i byte for byte _container(syms[i], H, W): the tiles of
        all volumes coded by one launch per tile shape (format 1: the volumes of one shape by one launch).  The tail of
        compress_many and of transcode_many."""
        import torch
        if not self.device_encode:
            return [self._container(sym, H, W) for sym, (H, W) in zip(syms, sizes)]
        row, param = self._target()
        if row.version != FORMAT_VERSION:
            coded = self.pred.encode_tiles_batch(syms, self.tile[0], self.tile[1], **_coder_kw(row, param))
            return [self._pack(row, param, coded[i], syms[i], H, W) for i, (H, W) in enumerate(sizes)]
        out = [None] * len(syms)
        by_shape = {}
        for i, sym in enumerate(syms):
            by_shape.setdefault(tuple(sym.shape), []).append(i)
        for shape, members in by_shape.items():          # format 1: volumes of one shape are one encode_stream batch
            C, h, w = (int(v) for v in shape)
            for i, (payload, first_sym) in zip(members, self.pred.encode_stream(torch.stack([syms[i] for i in members]))):
                out[i] = build_container(self.ae_name, self.pc_name, sizes[i][0], sizes[i][1], C, h, w, self.L, first_sym,
                                         self.pred.freqs_resolution, self.fingerprint, payload)
        return out

    def _crop(self, x_out_chw, c):
        img = np.transpose(x_out_chw.cpu().numpy(), (1, 2, 0))
        f = self.factor
        t, l = ((-c.H) % f) // 2, ((-c.W) % f) // 2                               # val.add_padding's offsets
        return np.ascontiguousarray(img[t:t + c.H, l:l + c.W, :])

    def _decode_together(self, heads, want, max_workspace_bytes=1 << 31, channels=None):
        """the batched part of decompress_many / transcode_many over parsed and checked containers: per kind (raster, wavefront,
        layered, front-layered) the tiled files of the most frequent tile extent (and layer ends) in one decode_tiles_batch call ->
        yields (their indices, per file q or symbols on the device); the other files are the caller's, one by one"""
        keys = [_batch_key(c) if isinstance(c, _TILED) else None for c in heads]
        for kind in dict.fromkeys((row.order, row.param_kw) for row in FORMATS.values() if row.container in _TILED):
            mine = [i for i, key in enumerate(keys) if key is not None and key[2:4] == kind]
            extents = [keys[i] for i in mine]
            major = max(sorted(set(extents)), key=extents.count) if extents else None
            together = [i for i, e in zip(mine, extents) if e == major]
            if not together:
                continue
            try:
                got = self.pred.decode_tiles_batch([(heads[i].streams, heads[i].first_syms, (heads[i].C, heads[i].h, heads[i].w))
                                                    for i in together], major[0], major[1], want=want,
                                                   max_workspace_bytes=max_workspace_bytes, channels=channels,
                                                   **_decode_kw(heads[together[0]]))
            except ValueError as e:
                m = re.search(r'volume (\d+)', str(e))
                where = 'file {}: '.format(together[int(m.group(1))]) if m else ''
                raise ValueError('{}decoder status is not 0: {}'.format(where, e))
            yield together, got

    def decompress_many(self, datas, max_workspace_bytes=1 << 31, channels=None):
        """[container bytes] of either format, any mix of shapes -> [HWC uint8], element i equal to decompress(datas[i]); with
        channels=K to decompress(datas[i], channels=K), one K for the call.
        Every file is parsed and checked first; the first refusal raises its ValueError with the index of the file in front and
        nothing has reached the device.  The format-2 / format-4 files of the most frequent tile extent are decoded together
        (decode_tiles_batch: the tiles of all of them in one launch per workspace chunk, the centres q staying on the device) and
        go through the decoder up to IN_FLIGHT at a time; so are, in launches of their own (the order is a flag of the call), the
        format-5 files of their most frequent extent, and the format-6 and the format-8 files of their most frequent (tile extent,
        layer ends) each;
        format-1 files and the other tiled files take the single-file path."""
        import torch
        channels = check_channels(channels, self.C)
        heads = []
        for i, data in enumerate(datas):
            try:
                c = parse_container(data)
                self.check_container(c)
            except ValueError as e:
                raise ValueError('file {}: {}'.format(i, e))
            heads.append(c)
        out = [None] * len(datas)
        for together, qs in self._decode_together(heads, 'q', max_workspace_bytes, channels):
            imgs = self._in_flight(qs, lambda ae, q: ae.decode(q[None], is_training=False).to(torch.uint8)[0])    # tf.cast truncates (val.py)
            for i, x in zip(together, imgs):
                out[i] = self._crop(x, heads[i])
        for i, data in enumerate(datas):
            if out[i] is None:
                try:
                    out[i] = self.decompress(data, channels=channels)
                except ValueError as e:
                    raise ValueError('file {}: {}'.format(i, e))
        return out

    # -- a pixel rectangle of a tiled file, from the tiles it needs --

    def region_plan(self, c, rect):
        """region_plan for a parsed tiled container with this model's reach under the kernels the whole picture runs
        (Autoencoder.decode_family): decoder_reach where the 3 x 3 layers run the direct or the F(2x2) form, the wider decoder_cells
        where they or h12 run F(4x4), whose transforms carry the rounding of a tile's other inputs into an output -- about 32 cells
        a side instead of 17 for B = 5.  align = 2: the window begins at an even cell, a multiple of 4 positions at H/4, so the
        4 x 4 tiles of the F(4x4) kernels fall where the whole picture has them."""
        B = int(self.ae.config.arch_param_B)
        form, _, h12_w4 = self.ae.decode_family(c.h * self.factor, c.w * self.factor)
        reach = (lambda p0, p1: decoder_cells(p0, p1, B, form == 2, h12_w4)) if form == 2 or h12_w4 else decoder_reach(B)
        return region_plan(c.H, c.W, self.factor, c.h, c.w, c.th, c.tw, rect, reach, align=2)

    def _region_head(self, data, rect):
        """one request, on the host: the whole file parsed and checked as decompress does -> (container, RegionPlan, window container
        or None, plan bits).  The window container is the file cut to the plan's tiles -- (h, w), streams and first symbols -- which is
        all a decoder reads of it; None: the whole picture is decoded and cropped, because the rectangle needs every tile or because
        the window cannot have the kernel family of the whole picture (Autoencoder.plan_like / plan_holds)."""
        c = parse_container(data)
        self.check_container(c)
        if not isinstance(c, _TILED):
            raise ValueError('region decode needs tiles: a format-{} file is one stream over the whole volume and decodes only as a '
                             'whole; write it with --tile'.format(c.version))
        plan = self.region_plan(c, rect)
        f = self.factor
        y0, x0, wh, ww = plan.window
        if (wh, ww) == (c.h, c.w):
            return c, plan, None, 0
        bits = self.ae.plan_like(c.h * f, c.w * f)
        if not self.ae.plan_holds(bits, c.h * f, c.w * f, wh * f, ww * f, y0 * f, x0 * f):
            return c, plan, None, 0
        return c, plan, c._replace(h=wh, w=ww, streams=[c.streams[t] for t in plan.tiles],
                                   first_syms=[c.first_syms[t] for t in plan.tiles]), bits

    @staticmethod
    def _region_crop(img_hwc, plan):
        x, y, rw, rh = plan.rect
        return np.ascontiguousarray(img_hwc[y:y + rh, x:x + rw, :])

    def _window_pixels(self, ae, q, plan, bits):
        """q (C, wh, ww) of a window on the device -> the rectangle's (3, rh, rw) uint8 pixels, still there"""
        import torch
        x_out = ae.decode(q[None], is_training=False, plan_flags=bits).to(torch.uint8)[0]      # tf.cast truncates (val.py)
        (oy, ox), (_, _, rw, rh) = plan.offset, plan.rect
        return x_out[:, oy:oy + rh, ox:ox + rw].contiguous()

    def decompress_region(self, data, rect, channels=None):
        """container bytes of a tiled file (formats 2, 4, 5, 6, 8, 10), rect = (x, y, w, h) in pixels of the image (clipped to it, as
        --roi's) -> the HWC uint8 pixels of the rectangle, bit for bit decompress(data)[y:y + h, x:x + w]; with channels=K those of
        decompress(data, channels=K).
        The whole file is parsed and checked as decompress does -- sizes, every CRC, the model -- so a damaged file is refused
        wherever the damage lies.  Then only the tiles whose cells the rectangle's pixels depend on (region_plan, decoder_reach)
        are entropy-decoded, as a volume of their own (decode_tiles_batch, q staying on the device), and the autoencoder's decoder
        runs over that window alone.
        The kernels of the whole picture are forced on the window (Autoencoder.plan_like): the 3 x 3 layers' form and h12's depend on
        the shape and round differently.  Forcing alone does not suffice for an F(4x4) picture: its transforms carry the rounding of
        a tile's other inputs into an output, so the window is that of decoder_cells there, about 34 cells a side instead of 18
        (Codec.region_plan); with it the window's values are the picture's bit for bit before the cast.  Where the form cannot be
        had the WHOLE picture is decoded and cropped -- never other pixels: a rectangle that needs every tile; an F(4x4) picture
        whose window's width at H/4 is no multiple of 4 (an odd number of cells: odd tile extents only); a picture whose automatic
        F(2x2) plan mixes whole-K and K-split launches (256 or more tile groups at H/4 with a remainder that runs K-split); plan
        flags of this Codec that pin a decomposition or leave CUs idle; a picture of 2^25 pixels or more.
        A ValueError for format 1 (it names --tile), for a rectangle of no extent or one that misses the image, and for everything
        decompress refuses."""
        channels = check_channels(channels, self.C)
        c, plan, win, bits = self._region_head(data, rect)
        if win is None:
            return self._region_crop(self.decompress(data, channels=channels), plan)
        try:
            q = self.pred.decode_tiles_batch([(win.streams, win.first_syms, (win.C, win.h, win.w))], win.th, win.tw, want='q', channels=channels,
                                             **_decode_kw(win))[0]
        except ValueError as e:
            raise ValueError('decoder status is not 0: {}'.format(e))
        return np.transpose(self._window_pixels(self.ae, q, plan, bits).cpu().numpy(), (1, 2, 0)).copy()

    def decompress_regions_many(self, requests, max_workspace_bytes=1 << 31, channels=None):
        """[(container bytes, rect)] -> [HWC uint8], element i equal to decompress_region(*requests[i]) (with channels=K: to
        decompress_region(.., channels=K), one K for the call); the same file may be asked for more than once.
        Every file is parsed and checked first; the first refusal raises its ValueError with the index of the request in front
        and nothing has reached the device.  The windows are grouped as decompress_many groups files: per kind (raster,
        wavefront, layered, front-layered) those of the most frequent tile extent (and layer ends) are the volumes of ONE
        decode_tiles_batch call -- a request whose whole picture is needed is the volume of all its tiles -- and go through the
        decoder up to IN_FLIGHT at a time, each with the forced plan of its own picture; the other requests take
        decompress_region one by one."""
        channels = check_channels(channels, self.C)
        requests, heads = list(requests), []
        for i, req in enumerate(requests):
            try:
                data, rect = req
                heads.append(self._region_head(data, rect))
            except ValueError as e:
                raise ValueError('request {}: {}'.format(i, e))
        out = [None] * len(heads)
        try:
            for together, qs in self._decode_together([c if win is None else win for c, _, win, _ in heads], 'q', max_workspace_bytes, channels):
                jobs = []
                for i, q in zip(together, qs):
                    c, plan, win, bits = heads[i]
                    if win is None:                                  # the whole picture: the rectangle sits at the padding's offsets in it
                        f = self.factor
                        plan = plan._replace(offset=(plan.rect[1] + ((-c.H) % f) // 2, plan.rect[0] + ((-c.W) % f) // 2))
                    jobs.append((q, plan, bits))
                for i, x in zip(together, self._in_flight(jobs, lambda ae, job: self._window_pixels(ae, *job))):
                    out[i] = np.transpose(x.cpu().numpy(), (1, 2, 0)).copy()
        except ValueError as e:
            raise ValueError(re.sub(r'^file (\d+): ', r'request \1: ', str(e)))
        for i, (data, rect) in enumerate(requests):
            if out[i] is None:
                try:
                    out[i] = self.decompress_region(data, rect, channels=channels)
                except ValueError as e:
                    raise ValueError('request {}: {}'.format(i, e))
        return out

    # -- what a damaged format-4 file still holds --

    def _salvage_head(self, data):
        """parse_salvage + the model checks -> (CheckedContainer, {tile: reason}, file_crc_ok); nothing on the device"""
        c, damage, file_crc_ok = parse_salvage(data)
        self.check_container(c)
        return c, dict(damage), file_crc_ok

    def _report(self, c, reasons, decoded, file_crc_ok):
        """reasons: {tile: 'crc' | 'truncated'} of the reader; decoded: [(tile, reason)] of decode_tiles_batch(conceal=True)"""
        f = self.factor
        top, left = ((-c.H) % f) // 2, ((-c.W) % f) // 2                         # val.add_padding's offsets
        grid, damaged = tile_grid(c.h, c.w, c.th, c.tw), []
        for t, why in decoded:
            y0, x0, a, b = grid[t]
            py0, py1 = min(max(y0 * f - top, 0), c.H), min(max((y0 + a) * f - top, 0), c.H)
            px0, px1 = min(max(x0 * f - left, 0), c.W), min(max((x0 + b) * f - left, 0), c.W)
            damaged.append(DamagedTile(t, reasons.get(t, why), (y0, x0, a, b), (py0, px0, py1 - py0, px1 - px0)))
        return SalvageReport(len(grid), bool(file_crc_ok), damaged)

    def salvage(self, data):
        """container bytes of format 4 or 5, possibly damaged -> (HWC uint8 image, SalvageReport).  Tiles whose bytes are there and match
        their CRC are decoded; the others -- and any whose decoder status is not 0 -- are filled on the device from their intact
        neighbours (ic_pc_conceal_tiles) and listed in report.damaged.  An intact file gives decompress(data) and an empty list.
        A ValueError where nothing can be recovered: another format, a damaged header, another model."""
        import torch
        c, reasons, file_crc_ok = self._salvage_head(data)
        qs, damage = self.pred.decode_tiles_batch([(c.streams, c.first_syms, (c.C, c.h, c.w))], c.th, c.tw, want='q', conceal=True,
                                                  **_decode_kw(c))
        x_out = self.ae.decode(qs[0][None], is_training=False).to(torch.uint8)   # tf.cast truncates (val.py)
        return self._crop(x_out[0], c), self._report(c, reasons, damage[0], file_crc_ok)

    def salvage_many(self, datas, max_workspace_bytes=1 << 31):
        """[container bytes of format 4 or 5] -> [(image, SalvageReport)], element i equal to salvage(datas[i]).  As decompress_many:
        every file is parsed and checked first (the first refusal raises with the index of the file in front, nothing has reached
        the device); then per tile extent and order the intact tiles of all files in one decode launch per workspace chunk, one concealment
        launch, q staying on the device, and the autoencoder passes up to IN_FLIGHT at a time."""
        import torch
        heads = []
        for i, data in enumerate(datas):
            try:
                heads.append(self._salvage_head(data))
            except ValueError as e:
                raise ValueError('file {}: {}'.format(i, e))
        out = [None] * len(datas)
        for extent in sorted(set(_batch_key(c) for c, _, _ in heads)):
            members = [i for i, (c, _, _) in enumerate(heads) if _batch_key(c) == extent]
            qs, damage = self.pred.decode_tiles_batch([(heads[i][0].streams, heads[i][0].first_syms, (heads[i][0].C, heads[i][0].h, heads[i][0].w))
                                                       for i in members], extent[0], extent[1], want='q', conceal=True,
                                                      max_workspace_bytes=max_workspace_bytes, **_decode_kw(heads[members[0]][0]))
            imgs = self._in_flight(qs, lambda ae, q: ae.decode(q[None], is_training=False).to(torch.uint8)[0])    # tf.cast truncates (val.py)
            for i, x, dmg in zip(members, imgs, damage):
                c, reasons, file_crc_ok = heads[i]
                out[i] = (self._crop(x, c), self._report(c, reasons, dmg, file_crc_ok))
        return out

    # -- what a damaged or cut format-6 file still holds, tile by tile --

    def _recover_head(self, data):
        """parse_recover + the model checks -> (LayeredContainer, layers per tile, {tile: reason}, file_crc_ok); nothing on the device"""
        c, layers, reasons, file_crc_ok = parse_recover(data)
        self.check_container(c)
        return c, layers, reasons, file_crc_ok

    def _recover_decode(self, heads, want, max_workspace_bytes=1 << 31):
        """heads of one (tile extent, layer ends) -> decode_tiles_batch(tile_layers=...): (per file q or symbols on the device, per file
        the tiles with fewer than C channels)"""
        c0 = heads[0][0]
        return self.pred.decode_tiles_batch([(c.streams, c.first_syms, (c.C, c.h, c.w)) for c, _, _, _ in heads], c0.th, c0.tw, want=want,
                                            max_workspace_bytes=max_workspace_bytes,
                                            tile_layers=[layers for _, layers, _, _ in heads], **_decode_kw(c0))

    def _recover_report(self, head, held):
        """held: [(tile, layers_read, channels, reason)] of decode_tiles_batch(tile_layers=...); the reader's reason where it has one"""
        c, _, reasons, file_crc_ok = head
        f = self.factor
        top, left = ((-c.H) % f) // 2, ((-c.W) % f) // 2                         # val.add_padding's offsets
        grid, tiles = tile_grid(c.h, c.w, c.th, c.tw), []
        for t, layers, channels, why in held:
            y0, x0, a, b = grid[t]
            py0, py1 = min(max(y0 * f - top, 0), c.H), min(max((y0 + a) * f - top, 0), c.H)
            px0, px1 = min(max(x0 * f - left, 0), c.W), min(max((x0 + b) * f - left, 0), c.W)
            tiles.append(RecoveredTile(t, layers, channels, why or reasons[t], (y0, x0, a, b), (py0, px0, py1 - py0, px1 - px0)))
        return RecoverReport(len(grid), len(c.layer_ends), bool(file_crc_ok), tiles)

    def recover_symbols(self, data):
        """format-6 bytes, whole, cut or damaged -> (symbols (C,h,w) int64 numpy, LayeredContainer, RecoverReport): every tile's leading
        intact layers decoded, every missing (tile, channel) filled from the neighbours that hold it (the rule: tests/recover_rule.py)"""
        head = self._recover_head(data)
        syms, held = self._recover_decode([head], 'symbols')
        return syms[0].cpu().numpy(), head[0], self._recover_report(head, held[0])

    def recover(self, data):
        """format-6 bytes, whole, cut or damaged -> (HWC uint8 image, RecoverReport).  An intact file gives decompress(data) and an
        empty list; a file cut at a layer end gives decompress_partial(data)'s image.  A ValueError where nothing can be read:
        another format, a damaged header, another model."""
        import torch
        head = self._recover_head(data)
        qs, held = self._recover_decode([head], 'q')
        x_out = self.ae.decode(qs[0][None], is_training=False).to(torch.uint8)   # tf.cast truncates (val.py)
        return self._crop(x_out[0], head[0]), self._recover_report(head, held[0])

    def recover_many(self, datas, max_workspace_bytes=1 << 31):
        """[format-6 bytes] -> [(image, RecoverReport)], element i equal to recover(datas[i]).  As salvage_many: every file is parsed
        and checked first (the first refusal raises with the index of the file in front, nothing has reached the device); then per
        (tile extent, layer ends) the tiles of all files in one decode launch per workspace chunk, one concealment launch, q staying
        on the device, and the autoencoder passes up to IN_FLIGHT at a time."""
        import torch
        heads = []
        for i, data in enumerate(datas):
            try:
                heads.append(self._recover_head(data))
            except ValueError as e:
                raise ValueError('file {}: {}'.format(i, e))
        out = [None] * len(datas)
        kind = lambda c: (c.version, c.th, c.tw) + tuple(c.layer_ends)
        for group in sorted(set(kind(h[0]) for h in heads)):
            members = [i for i, h in enumerate(heads) if kind(h[0]) == group]
            qs, held = self._recover_decode([heads[i] for i in members], 'q', max_workspace_bytes)
            imgs = self._in_flight(qs, lambda ae, q: ae.decode(q[None], is_training=False).to(torch.uint8)[0])    # tf.cast truncates (val.py)
            for i, x, tiles in zip(members, imgs, held):
                out[i] = (self._crop(x, heads[i][0]), self._recover_report(heads[i], tiles))
        return out

    # -- a file to a file: another format, a lower rate, no image and no autoencoder --

    def _keep_plane(self, c, cap=None, rois=None, background=None):
        """transcode's cap arguments for the file of container c -> None (no cap) or the (h, w) int64 plane of channels kept per
        cell (cap_plane on the header's H, W, then cap_channels: integer levels only)"""
        if cap is None and not rois and background is None:
            return None
        return cap_channels(self.cap_plane(c.H, c.W, cap, rois, background), c.C)

    def _capped(self, sym, keep):
        """cap_symbols on the device: sym (C, h, w) int64, keep None or the (h, w) int64 plane of _keep_plane"""
        import torch
        if keep is None or int(keep.min()) >= int(sym.shape[0]):
            return sym
        k = torch.as_tensor(keep).to(sym.device)
        below = torch.arange(int(sym.shape[0]), device=sym.device)[:, None, None] < k[None]
        return torch.where(below, sym, torch.full_like(sym, self.pred.conceal_fallback()))

    def _decode_device(self, c):
        """a parsed and checked container -> its (C, h, w) int64 symbols, left on the device"""
        shape = (c.C, c.h, c.w)
        try:
            if isinstance(c, _TILED):
                return self.pred.decode_tiles_batch([(c.streams, c.first_syms, shape)], c.th, c.tw, want='symbols', **_decode_kw(c))[0]
            return self.pred.decode_stream(c.payload, shape, c.first_sym, on_device=True)
        except ValueError as e:
            raise ValueError('decoder status is not 0: {}'.format(str(e).replace('(volume 0, tile ', '(tile ')))

    def transcode(self, data, cap=None, rois=None, background=None):
        """container bytes of any format -> container bytes in the format THIS Codec writes (tile, checked, order, layers,
        front_layers), byte for byte what compress would have written for the image: the symbols are decoded and left on the device,
        then coded again; the autoencoder is not run, so nothing is lost a second time.  cap, rois, background: as compress takes them,
        but at integer levels only (cap_channels: a fractional cap needs the bottleneck) -- cell p keeps the channels below its level,
        the others get the fill symbol (cap_symbols), which is compress(img, cap=...) of the same levels.  The file is parsed and
        checked as decompress does it; every refusal, the target format's included, comes before any device work."""
        self._target()
        c = parse_container(data)
        self.check_container(c)
        keep = self._keep_plane(c, cap, rois, background)
        return self._container(self._capped(self._decode_device(c), keep), c.H, c.W)

    def transcode_many(self, datas, caps=None, max_workspace_bytes=1 << 31):
        """[container bytes] of any mix of formats and shapes -> [container bytes], element i equal to transcode(datas[i], cap=caps[i])
        (caps: None, or one entry per file -- None, an integer level or a plane).  Every file is parsed and checked first: the first
        refusal raises its ValueError with 'file i: ' in front and nothing has reached the device.  The sources are grouped as
        decompress_many groups them (per kind the files of the most frequent tile extent / layer ends in one decode launch per
        workspace chunk, the others file by file), the symbols stay on the device, and the targets are coded as compress_many codes
        them: the tiles of all files in one launch per tile shape."""
        datas = list(datas)
        caps = [None] * len(datas) if caps is None else list(caps)
        if len(caps) != len(datas):
            raise ValueError('caps: {} entries for {} files'.format(len(caps), len(datas)))
        self._target()
        heads, keeps = [], []
        for i, (data, cap) in enumerate(zip(datas, caps)):
            try:
                c = parse_container(data)
                self.check_container(c)
                keeps.append(self._keep_plane(c, cap))
            except ValueError as e:
                raise ValueError('file {}: {}'.format(i, e))
            heads.append(c)
        syms = [None] * len(datas)
        for together, got in self._decode_together(heads, 'symbols', max_workspace_bytes):
            for i, sym in zip(together, got):
                syms[i] = sym
        for i, c in enumerate(heads):
            if syms[i] is None:
                try:
                    syms[i] = self._decode_device(c)
                except ValueError as e:
                    raise ValueError('file {}: {}'.format(i, e))
        return self._containers([self._capped(sym, keep) for sym, keep in zip(syms, keeps)], [(c.H, c.W) for c in heads])

    def transcode_to_budget(self, data, max_bytes, rois=None):
        """the largest integer level K in 0 .. C whose file has at most max_bytes bytes -> (out, K, probes): out is byte for byte
        transcode(data, cap=K), or with rois transcode(data, rois=rois, background=K) (the rectangles stay uncapped, the budget is
        met by the background); probes is the number of real codings.  The file is decoded once; every level after that is one
        torch.where over its symbols.  An estimate from the context model's bit costs (up to 16 capped volumes a launch, one
        readback a round) starts budget_search(steps=C), whose contract holds on the real files: out fits, and the file of K + 1
        does not (or K == C) -- at most 1 + 2 + 1 + ceil(log2 C) codings.  A ValueError if the file of level 0 is over the budget."""
        import torch
        from ._lib import lib, check, ptr, current_stream
        max_bytes = int(max_bytes)
        self._target()
        c = parse_container(data)
        self.check_container(c)
        C = self.C
        roi = np.isinf(cap_plane(c.H, c.W, self.factor, rois=rois, background=0.0)) if rois else None
        sym = self._decode_device(c)
        planes = lambda k: np.full((c.h, c.w), k, np.int64) if roi is None else np.where(roi, C, k).astype(np.int64)
        files = {}

        def coded(k):
            if k not in files:
                files[k] = self._container(self._capped(sym, planes(k)), c.H, c.W)
            return files[k]

        def estimate(ks):                                             # bytes of the whole-volume pass per level, one readback
            vols = torch.stack([self._capped(sym, planes(k)) for k in ks])
            q = self.ae.get_centers_variable()[vols].contiguous()
            bits = self.pc.bitcost(q, vols, is_training=False, pad_value=self.pc.auto_pad_value(self.ae))
            buf = torch.empty(1024 + len(ks), dtype=torch.float32, device=self.device)
            check(lib.ic_mean_rows_f32(ptr(bits), len(ks), bits.numel() // len(ks), 8.0, ptr(buf), ptr(buf[1024:]),
                                       current_stream(self.device)), 'ic_mean_rows_f32')
            return [float(v) for v in buf[1024:].cpu().numpy()]

        guess = C
        if len(coded(C)) > max_bytes and C > 1:
            # the container and the streams' ends cost the same at every level, to first order: take them from the one real file
            step = (C + 15) // 16
            ks = list(range(step, C + 1, step))
            if ks[-1] != C:
                ks[-1] = C
            est = estimate(ks)
            room = max_bytes - (len(files[C]) - est[-1])
            below = [k for k, b in zip(ks, est) if b <= room]
            ks = list(range(1, step)) if not below else list(range(below[-1] + 1, min(below[-1] + step, C)))
            guess = below[-1] if below else 0
            if ks:
                fit = [k for k, b in zip(ks, estimate(ks)) if b <= room]
                guess = fit[-1] if fit else guess
        try:
            k, probes = budget_search(lambda k: len(coded(k)) <= max_bytes, guess, steps=C)
        except ValueError:
            raise ValueError('budget of {} bytes: the smallest file, at level 0, has {} bytes'.format(max_bytes, len(coded(0))))
        return files[k], int(k), probes

    def repair(self, data, cap=None):
        """what a damaged or cut file still holds, written as an intact file in the format this Codec writes -> (bytes, report).  A
        format-4 / format-5 source is read as salvage reads it (the intact tiles decoded, the others filled from their neighbours by
        ic_pc_conceal_tiles; report: salvage's SalvageReport), a format-6 / format-8 source as recover reads it (recover_symbols;
        report: recover's RecoverReport); the symbols stay on the device and are coded again, under `cap` if one is given (as
        transcode's).  decompress(out) is salvage's / recover's picture; an intact file gives transcode(data) and an empty list.
        Formats 1 and 2 carry no checksums to read a damaged file by: refused in salvage's words."""
        self._target()
        raw = bytes(data)
        _refuse(raw, 'repair')
        if _source_version(raw) in _LAYERED_VERSIONS:
            head = self._recover_head(raw)
            c = head[0]
            keep = self._keep_plane(c, cap)
            syms, held = self._recover_decode([head], 'symbols')
            report = self._recover_report(head, held[0])
        else:
            c, reasons, file_crc_ok = self._salvage_head(raw)
            keep = self._keep_plane(c, cap)
            syms, damage = self.pred.decode_tiles_batch([(c.streams, c.first_syms, (c.C, c.h, c.w))], c.th, c.tw, want='symbols', conceal=True,
                                                        **_decode_kw(c))
            report = self._report(c, reasons, damage[0], file_crc_ok)
        return self._container(self._capped(syms[0], keep), c.H, c.W), report

    # -- the other axis: what a file, a level, a target costs in picture quality --

    def _original(self, img_hw3_uint8):
        """(H, W, 3) uint8 numpy -> the (1, 3, H, W) uint8 device tensor the metrics take: the one upload of a measure"""
        import torch
        return torch.as_tensor(np.ascontiguousarray(np.transpose(img_hw3_uint8, (2, 0, 1)))[None]).to(self.device)

    def _values(self, orig, pic, box=None):
        """orig (1, 3, H, W) and pic (3, H, W), uint8 on the device; box None or (x0, y0, x1, y1) -> the six float64 values of
        metrics.val_metrics_device as one device tensor (scale values, then the mean squared error), nothing waited for"""
        import torch
        from . import metrics
        pic = pic[None]
        if box is not None:
            x0, y0, x1, y1 = box
            orig, pic = orig[:, :, y0:y1, x0:x1], pic[:, :, y0:y1, x0:x1]
        scales, mse = metrics.val_metrics_device(orig.contiguous(), pic.contiguous())
        return torch.cat([scales, mse.reshape(1)])

    def written_version(self):
        """the format version of the files this Codec writes (its refusals are _target's)"""
        return self._target()[0].version

    def measure(self, img_hwc_uint8, data, channels=None, rect=None):
        """how good is this file?  -> Measure(bytes, bpp, mse, psnr, ms_ssim) of decompress(data, channels=channels) against its
        original img: the decoded picture stays on the device, the original is uploaded once, and both go through
        metrics.val_metrics_device (float64, the operations of the NumPy code val.py reports) -- measure_from_values says how the
        fields follow.  bytes and bpp are the whole file's, header included: bpp = 8 len(data) / (H W).  rect = (x, y, w, h): the
        metrics of that pixel rectangle of both pictures, clipped to the image as a region of interest is; bytes and bpp stay the
        file's.  data is read as decompress reads it and refused as decompress refuses it; a ValueError too for an img of another
        shape than the file's picture and for a rectangle of which less than 16 pixels a side lie in the image."""
        sym, c = self.decode_symbols(data, channels=channels)
        img = check_measured_image(img_hwc_uint8, c.H, c.W)
        box = None if rect is None else measure_rect(rect, c.H, c.W)
        values = self._values(self._original(img), self._picture(sym, c.H, c.W), box)
        return measure_from_values(values.tolist(), len(data), c.H * c.W)

    def _cap_planes(self, H, W, levels, rois=None):
        """(1, T, h, w) float32 on the device for requantize: per level the plane compress(cap=level) builds, or with rois the one
        of compress(rois=rois, background=level)"""
        import torch
        planes = [self.cap_plane(H, W, None, rois, lv) if rois else self.cap_plane(H, W, lv) for lv in levels]
        return torch.as_tensor(np.stack(planes)[None]).to(self.device)

    def _quality_inputs(self, img_hwc_uint8):
        """the part of rd_curve and compress_to_quality that runs once per image -> (bottleneck, original on the device, (H, W))"""
        x, (H, W) = self._image_tensor(img_hwc_uint8)
        self._target()
        _, bott = self.ae.encode_capped(x, None, keep_bottleneck=True)
        return bott, self._original(np.asarray(img_hwc_uint8)[:, :, :3]), (H, W)

    def compress_counting(self, img_hwc_uint8, rdo, cap=None, rois=None, background=None):
        """compress(img, rdo=rdo, ...) -> (data, the number of symbols that differ from the quantiser's, the number of symbols)"""
        sym, enc, (H, W) = self.choose_symbols(img_hwc_uint8, rdo, cap=cap, rois=rois, background=background)
        return self._container(sym, H, W), int((sym != enc.symbols[0]).sum()), int(sym.numel())

    def rdo_curve(self, img_hwc_uint8, lambdas):
        """what does a lambda cost in quality, and save in bytes, on this picture?  -> [(lambda, Measure)], row i equal in every field
        to measure(img, compress(img, rdo=lambdas[i])).  lambdas: a non-empty sequence of numbers, 0 <= lambda < inf.  The encoder
        runs once, as compress runs it; all lambdas are swept by one chooser launch per chunk, each coded to a real file in this
        Codec's format, and each decoded by a batch-1 pass of its own, as rd_curve does."""
        import torch
        lambdas = [check_rdo(v) for v in list(lambdas)]
        if not lambdas:
            raise ValueError('rdo_curve: no lambda given')
        if self.rdo_refusal:
            raise ValueError(self.rdo_refusal)
        self._target()
        enc, (H, W) = self.encode_symbols(img_hwc_uint8)
        orig = self._original(np.asarray(img_hwc_uint8)[:, :, :3])
        z = enc.z[0].contiguous()
        th, tw = self._rdo_tile(z.shape[1], z.shape[2])
        sizes, values = [], []
        for start in range(0, len(lambdas), 16):
            part = lambdas[start:start + 16]
            syms = self.pred.choose_tiles_batch([z] * len(part), th, tw, part)
            sizes += [len(d) for d in self._containers(syms, [(H, W)] * len(part))]
            pics = self._in_flight(syms, lambda ae, s: self._picture(s, H, W, ae))
            values += [self._values(orig, pic) for pic in pics]
        return [(lm, measure_from_values(v, n, H * W)) for lm, n, v in zip(lambdas, sizes, torch.stack(values).tolist())]

    def rd_curve(self, img_hwc_uint8, levels=None, rois=None):
        """what does a cap level cost in quality on this picture?  -> [(level, Measure)], row i equal in every field to
        measure(img, compress(img, cap=levels[i])) -- with rois to measure(img, compress(img, rois=rois, background=levels[i])), the
        rectangles uncapped as in compress_to_budget.  levels: None (rd_levels(C): the 17 levels k C / 16) or a non-empty increasing
        sequence of levels.  The encoder runs once; the levels are requantised from its bottleneck 16 a launch, each coded to a real
        file in this Codec's format (the tiles of a launch's levels by one coder launch per tile shape), and each decoded by a
        batch-1 pass of its own, up to IN_FLIGHT at a time: the kernel form of a layer depends on the batch size, and a batch of
        levels might run one that rounds differently from decompress's."""
        levels = check_rd_levels(levels, self.C)
        bott, orig, (H, W) = self._quality_inputs(img_hwc_uint8)
        sizes, values = [], []
        for start in range(0, len(levels), 16):
            part = levels[start:start + 16]
            syms = list(self.ae.requantize(bott, self._cap_planes(H, W, part, rois), hard_only=True).symbols)
            sizes += [len(d) for d in self._containers(syms, [(H, W)] * len(part))]
            pics = self._in_flight(syms, lambda ae, s: self._picture(s, H, W, ae))
            values += [self._values(orig, pic) for pic in pics]
        import torch
        return [(lv, measure_from_values(v, n, H * W)) for lv, n, v in zip(levels, sizes, torch.stack(values).tolist())]

    def compress_to_quality(self, img_hwc_uint8, psnr=None, ms_ssim=None, rois=None):
        """give me the smallest level that still reaches the target -> (data, level, Measure, probes).  Exactly one of psnr (dB) and
        ms_ssim (0 .. 1) is the target.  The search runs over cap_levels(C), the grid of compress_to_budget; a probe is one
        requantisation of the kept bottleneck, one batch-1 decode and one metrics call -- nothing is entropy-coded to probe.
        quality_search's contract holds on the measured pictures: data -- byte for byte compress(img, cap=level), with rois
        compress(img, rois=rois, background=level) -- meets the target, Measure == measure(img, data), and the next level down misses
        it (or level == 0); a nan never meets a target; probes <= 1 + 2 + 8.  A ValueError, which says what the file without a cap
        reaches, if that file misses the target."""
        name, target = quality_target(psnr, ms_ssim)
        bott, orig, (H, W) = self._quality_inputs(img_hwc_uint8)
        levels = cap_levels(self.C)
        probed = {}

        def meets(k):
            sym = self.ae.requantize(bott, self._cap_planes(H, W, [levels[k]], rois), hard_only=True).symbols[0]
            probed[k] = (sym, measure_from_values(self._values(orig, self._picture(sym, H, W)).tolist(), 0, H * W))
            return meets_target(probed[k][1], name, target)

        try:
            k, probes = quality_search(meets, CAP_STEPS)
        except ValueError:
            if CAP_STEPS not in probed or meets_target(probed[CAP_STEPS][1], name, target):
                raise
            raise ValueError('{} target {:g}: the file without a cap reaches {:g}'.format(name, target, getattr(probed[CAP_STEPS][1], name)))
        data = self._container(probed[k][0], H, W)
        return data, float(levels[k]), probed[k][1]._replace(bytes=len(data), bpp=8.0 * len(data) / (H * W)), probes

    def transcode_to_quality(self, data, psnr=None, ms_ssim=None):
        """a file to a file of lower rate, as far as its picture stays within the target OF THE PICTURE THE FILE DECODES TO NOW
        -> (out, K, Measure, probes): the smallest integer level K in 0 .. C, in quality_search's sense, whose picture measured
        against decompress(data) meets the target; out is byte for byte transcode(data, cap=K), Measure its measure against
        decompress(data).  The symbols are decoded once and stay on the device; a probe is one torch.where over them (cap_symbols),
        one batch-1 decode and one metrics call; the encoder is never run.  Level C is the file's own picture (psnr inf, ms_ssim 1)
        and meets every target, so probes <= 1 + 2 + ceil(log2 C)."""
        name, target = quality_target(psnr, ms_ssim)
        self._target()
        c = parse_container(data)
        self.check_container(c)
        sym = self._decode_device(c)
        orig = self._picture(sym, c.H, c.W)[None].contiguous()
        probed = {}

        def meets(k):
            capped = self._capped(sym, np.full((c.h, c.w), k, np.int64))
            probed[k] = (capped, measure_from_values(self._values(orig, self._picture(capped, c.H, c.W)).tolist(), 0, c.H * c.W))
            return meets_target(probed[k][1], name, target)

        K, probes = quality_search(meets, self.C)
        out = self._container(probed[K][0], c.H, c.W)
        return out, int(K), probed[K][1]._replace(bytes=len(out), bpp=8.0 * len(out) / (c.H * c.W)), probes

    def open_stream(self, max_workspace_bytes=1 << 31, fronts=False):
        """a StreamDecoder: a format-6 file fed as it arrives, recover's picture of the bytes so far, every layer decoded once;
        fronts=True: a format-8 file is taken as well, every front swept once"""
        return StreamDecoder(self, max_workspace_bytes, fronts=fronts)

    def compress_file(self, image_path, out_path, **cap_args):
        from PIL import Image
        img = np.asarray(Image.open(image_path).convert('RGB'), dtype=np.uint8)     # as val.load_image_chw reads it
        data = self.compress(img, **cap_args)
        with open(out_path, 'wb') as f:
            f.write(data)
        return data, img.shape[0] * img.shape[1]

    def decompress_file(self, in_path, image_path, channels=None):
        from PIL import Image
        channels = check_channels(channels, self.C)
        with open(in_path, 'rb') as f:
            data = f.read()
        img = self.decompress(data, channels=channels)
        Image.fromarray(img).save(image_path)
        return img


def _coder_kw(row, param):
    """what encode_tiles* and decode_tiles_batch are told for the tiled format `row` with its parameter (the layer ends or the extra field)"""
    kw = {} if row.order is None else {'order': row.order}
    if row.param_kw is not None:
        kw[row.param_kw] = param
    return kw


def _param(c):
    """the parameter of a parsed tiled container's format: its layer ends, its extra field, or None"""
    row = FORMATS[c.version]
    return c.layer_ends if row.layered else getattr(c, row.extra) if row.extra else None


def _decode_kw(c):
    """what decode_tiles_batch is told about the streams of a parsed tiled container"""
    return _coder_kw(FORMATS[c.version], _param(c))


_ends_kw = _decode_kw                                                # the name tests/test_gpu_codec_golden.py and tools/codec_fronts_timing.py call it by

def _batch_key(c):
    """tiled containers with one key decode in one decode_tiles_batch call: the tile extent, what the decoder is told (formats 2 and 4
    are one kind of stream) and the format's parameter"""
    row, param = FORMATS[c.version], _param(c)
    return (c.th, c.tw, row.order, row.param_kw, tuple(param) if row.layered else param)


class StreamDecoder(object):
    """a format-6 file that is still arriving (Codec.open_stream).
    feed(chunk): appends the bytes; False while the header is not whole, True once it is and passes its CRC and the model checks.  The
        ValueErrors of recover -- another format, a damaged header, another model -- are raised by the feed that shows them.
    progress(): the number of leading intact layers per tile in the bytes so far (parse_recover), () before the header; no device.
    image(): (HWC uint8 image, RecoverReport), equal to Codec.recover(the bytes so far).  The first call opens the session
        (PredictionNetwork.open_layers); every call decodes, per tile, only the layers gained since the last one, conceals per (tile,
        channel) and runs one autoencoder pass.  ValueError('no complete layer ...') while no tile has a layer.  Without a new layer in
        any tile the last picture is returned again and nothing is launched (the report is that of the bytes so far).
    fronts=True: a format-8 file is streamed as well, its session opened with the file's ends as front ends
        (ic_pc_decode_tiles_batch_fronts_resume_f32); a format-6 file streams as with fronts=False.  Without it a format-8 file is
        refused by the feed that shows its version."""

    def __init__(self, codec, max_workspace_bytes=1 << 31, fronts=False):
        self.codec, self.max_workspace_bytes, self.fronts = codec, int(max_workspace_bytes), bool(fronts)
        self._buf = bytearray()
        self._header = None            # its length, once known
        self._ready = False
        self._head = None              # (bytes fed, _recover_head of them)
        self._session = None
        self._last = None              # (layers, image, held) of the last picture

    @property
    def bytes_fed(self):
        return len(self._buf)

    def feed(self, chunk):
        self._buf += bytes(chunk)
        if self._ready:
            return True
        if self._header is None:
            self._header = stream_header_bytes(self._buf[:1 << 18], fronts=self.fronts)      # (the fields that give the length end below 2^18)
        if self._header is None or len(self._buf) < self._header:
            return False
        self._parsed()                 # the header's CRC, the model checks: raises what recover raises
        self._ready = True
        return True

    def _parsed(self):
        if self._head is None or self._head[0] != len(self._buf):
            self._head = (len(self._buf), self.codec._recover_head(bytes(self._buf)))
        return self._head[1]

    def progress(self):
        return tuple(self._parsed()[1]) if self._ready else ()

    def image(self):
        import torch
        if not self._ready:
            raise ValueError('no complete layer: the header is not whole yet, {} bytes so far'.format(len(self._buf)))
        head = self._parsed()
        c, layers = head[0], list(head[1])
        if not any(layers):
            raise ValueError('no complete layer: no tile holds its layer 0 in the {} bytes so far'.format(len(self._buf)))
        codec = self.codec
        if self._last is None or self._last[0] != layers:
            if self._session is None:
                self._session = codec.pred.open_layers([(c.C, c.h, c.w)], c.th, c.tw, max_workspace_bytes=self.max_workspace_bytes, **_decode_kw(c))
            qs, held = self._session.advance([(c.streams, c.first_syms)], [layers], want='q')
            x_out = codec.ae.decode(qs[0][None], is_training=False).to(torch.uint8)      # tf.cast truncates (val.py)
            self._last = (layers, codec._crop(x_out[0], c), held[0])
        return self._last[1], codec._recover_report(head, self._last[2])


def _resolve_config(arg, tree, env):
    from . import config_parser
    if os.path.isfile(arg):
        return arg
    base = os.environ.get(env, config_parser.builtin_config_path(tree))
    p = os.path.join(base, *arg.split('/'))
    if not os.path.isfile(p):
        raise ValueError('config {!r} not found (a file, or a name below {})'.format(arg, base))
    return p


def _compress_line(path, data, pixels):
    c = parse_container(data)
    payload = len(c.payload)
    tiles = ', {} tiles'.format(len(c.streams)) if isinstance(c, _TILED) else ''
    return '{}: {} bytes, payload {} bytes = {:.4f} bpp, file {:.4f} bpp{}'.format(
        path, len(data), payload, 8.0 * payload / pixels, 8.0 * len(data) / pixels, tiles)


def _decompress_line(path, img, size, channels=None, C=None):
    line = '{}: {} x {} from {} bytes = {:.4f} bpp'.format(path, img.shape[0], img.shape[1], size, 8.0 * size / (img.shape[0] * img.shape[1]))
    return line if channels is None else '{}, preview from {} of {} channels'.format(line, channels, C)


def _damage_line(path, report):
    """one line for a salvaged file: the damaged tiles and where they lie in the image"""
    if not report.damaged:
        return '{}: salvaged, all {} tiles intact, the CRC over the file is missing or wrong'.format(path, report.ntiles)
    return '{}: salvaged, {} of {} tiles damaged: {}'.format(path, len(report.damaged), report.ntiles, ', '.join(
        'tile {} ({}) pixels y {}..{} x {}..{}'.format(d.index, d.reason, d.pixels[0], d.pixels[0] + d.pixels[2], d.pixels[1],
                                                      d.pixels[1] + d.pixels[3]) for d in report.damaged))


def _recover_line(path, report):
    """one line for a recovered file: the tiles with fewer than all layers, what they hold and where they lie in the image"""
    crc = '' if report.file_crc_ok else ', the CRC over the file is missing or wrong'
    if not report.tiles:
        return '{}: recovered, all {} tiles hold all {} layers{}'.format(path, report.ntiles, report.layers_total, crc)
    return '{}: recovered, {} of {} tiles incomplete: {}{}'.format(path, len(report.tiles), report.ntiles, ', '.join(
        'tile {} ({}) layers {} of {} = {} channels, pixels y {}..{} x {}..{}'.format(
            d.index, d.reason, d.layers, report.layers_total, d.channels, d.pixels[0], d.pixels[0] + d.pixels[2], d.pixels[1],
            d.pixels[1] + d.pixels[3]) for d in report.tiles), crc)


TRANSCODE_COMMANDS = ('transcode', 'transcode-dir')
WRITING_COMMANDS = ('compress', 'compress-dir', 'rd') + TRANSCODE_COMMANDS          # the commands that take --tile and its choices


def check_option_args(flags):
    """--checked / --wavefront / --salvage / --channels / --layers / --progressive / --front-layers / --front-progressive / --partial /
    --recover / --chunk / --fronts / --cap / --roi / --background / --max-bytes / --bpp / --region / --min-psnr / --min-ms-ssim /
    --levels / --rdo / --rdo-levels against the command, --tile and each other: decided before any model is built"""
    cap, background, rois = getattr(flags, 'cap', None), getattr(flags, 'background', None), getattr(flags, 'roi', None) or []
    max_bytes, bpp = getattr(flags, 'max_bytes', None), getattr(flags, 'bpp', None)
    transcoding = flags.command in TRANSCODE_COMMANDS
    for name, value in (('--cap', cap), ('--background', background), ('--max-bytes', max_bytes), ('--bpp', bpp)):
        if value is not None and flags.command not in ('compress', 'compress-dir') + TRANSCODE_COMMANDS:
            raise ValueError('{} belongs to compress / compress-dir: the cap on the importance map is the encoder\'s, a file is read '
                             'without it'.format(name))
    min_psnr, min_ms_ssim = getattr(flags, 'min_psnr', None), getattr(flags, 'min_ms_ssim', None)
    quality = '--min-psnr' if min_psnr is not None else '--min-ms-ssim' if min_ms_ssim is not None else None
    if quality is not None:
        if flags.command not in ('compress', 'compress-dir') + TRANSCODE_COMMANDS:
            raise ValueError('{} belongs to compress / compress-dir / transcode / transcode-dir: it searches for the level a file is '
                             'written at'.format(quality))
        if min_psnr is not None and min_ms_ssim is not None:
            raise ValueError('--min-psnr does not go with --min-ms-ssim: a search has one target')
        for name, value in (('--cap', cap), ('--max-bytes', max_bytes), ('--bpp', bpp), ('--background', background)):
            if value is not None:
                raise ValueError('{} does not go with {}: the quality target searches for the level'.format(quality, name))
        if transcoding and rois:
            raise ValueError('{} does not go with --roi here: a file is lowered to a quality at one level for every cell'.format(quality))
        for name in ('salvage', 'recover'):
            if getattr(flags, name, False):
                raise ValueError('{} does not go with --{}: a repaired file takes --cap alone'.format(quality, name))
        quality_target(min_psnr, min_ms_ssim)
    rdo, rdo_levels = getattr(flags, 'rdo', None), getattr(flags, 'rdo_levels', None)
    if rdo is not None:
        if transcoding:
            raise ValueError('--rdo does not go with {}: the choice weighs a symbol against the bottleneck value z, and a file has '
                             'no z'.format(flags.command))
        if flags.command not in ('compress', 'compress-dir'):
            raise ValueError('--rdo belongs to compress / compress-dir: the rate-aware choice of symbols is the encoder\'s, a file is '
                             'read without it')
        for name, value in (('--max-bytes', max_bytes), ('--bpp', bpp), ('--min-psnr', min_psnr), ('--min-ms-ssim', min_ms_ssim)):
            if value is not None:
                raise ValueError('--rdo does not go with {}: a search over lambda for a budget or a quality is not offered, the '
                                 'searches run over cap levels'.format(name))
        check_rdo(rdo)
    if rdo_levels is not None:
        if flags.command != 'rd':
            raise ValueError('--rdo-levels belongs to rd: the lambdas of the rate-distortion table\'s rows')
        if getattr(flags, 'levels', None) is not None or rois:
            raise ValueError('--rdo-levels does not go with --levels or --roi: its rows run over lambda in place of cap levels')
        parse_rdo_levels_arg(rdo_levels)
    if getattr(flags, 'levels', None) is not None:
        if flags.command != 'rd':
            raise ValueError('--levels belongs to rd: the number of steps of the rate-distortion table')
        rd_levels(1, flags.levels)
    if flags.command == 'measure' and getattr(flags, 'tile', None) is not None:
        raise ValueError('--tile belongs to compress / compress-dir: a file says by itself how it is tiled')
    if rois and flags.command == 'transcode-dir':
        raise ValueError('--roi belongs to compress / transcode: a rectangle is in the pixels of one image')
    if rois and flags.command not in ('compress', 'transcode', 'rd'):
        raise ValueError('--roi belongs to compress: a rectangle is in the pixels of one image' if flags.command == 'compress-dir' else
                         '--roi belongs to compress: the cap on the importance map is the encoder\'s, a file is read without it')
    if transcoding:
        for name, value in (('--cap', cap), ('--background', background)):
            if value is not None and _check_level(value, name) != float('inf') and float(value) != int(float(value)):
                raise ValueError('{} {:g} is not an integer: a fractional cap rescales z and needs the bottleneck, so it belongs to '
                                 'compress from the image; a file takes the integer levels 0 .. C'.format(name, float(value)))
        for name in ('salvage', 'recover'):
            if getattr(flags, name, False) and (rois or max_bytes is not None or bpp is not None):
                raise ValueError('--{} does not go with --roi, --max-bytes or --bpp: a repaired file takes --cap alone'.format(name))
    if max_bytes is not None and bpp is not None:
        raise ValueError('--max-bytes does not go with --bpp: the one names the budget in bytes, the other per pixel')
    if cap is not None and (max_bytes is not None or bpp is not None):
        raise ValueError('--cap does not go with {}: the one names the level, the other searches for it'.format(
            '--max-bytes' if max_bytes is not None else '--bpp'))
    if rois and background is None and max_bytes is None and bpp is None and quality is None and flags.command != 'rd':
        raise ValueError('--roi needs --background or a budget (--max-bytes / --bpp): the level of the cells outside the rectangles')
    if background is not None and not rois:
        raise ValueError('--background needs --roi: without a rectangle --cap is the level of every cell')
    if background is not None and (max_bytes is not None or bpp is not None):
        raise ValueError('--background does not go with {}: with --roi the budget searches for the background'.format(
            '--max-bytes' if max_bytes is not None else '--bpp'))
    for name, value in (('--cap', cap), ('--background', background)):
        if value is not None:
            _check_level(value, name)
    if max_bytes is not None and max_bytes < 1:
        raise ValueError('--max-bytes {} is not at least 1'.format(max_bytes))
    if bpp is not None and not bpp > 0:
        raise ValueError('--bpp {} is not above 0'.format(bpp))
    for r in rois:
        parse_roi_arg(r)
    if getattr(flags, 'chunk', None) is not None:
        if flags.command != 'stream':
            raise ValueError('--chunk belongs to stream: the size of the pieces the file is fed in')
        if flags.chunk < 1:
            raise ValueError('--chunk {} is not at least 1'.format(flags.chunk))
    if getattr(flags, 'fronts', False) and flags.command != 'stream':
        raise ValueError('--fronts belongs to stream: it lets a front-layered file (format 8) be streamed as well')
    if flags.command == 'stream':
        for name in ('salvage', 'partial', 'recover'):
            if getattr(flags, name, False):
                raise ValueError('--{} does not go with stream: it reads what has arrived of a layered file as --recover does, '
                                 'tile by tile'.format(name))
        if getattr(flags, 'channels', None) is not None:
            raise ValueError('--channels does not go with stream: what every tile holds so far decides its channels')
        if getattr(flags, 'tile', None) is not None:
            raise ValueError('--tile belongs to compress / compress-dir: a file says by itself how it is tiled')
    if getattr(flags, 'channels', None) is not None:
        if flags.command not in ('decompress', 'decompress-dir', 'measure'):
            raise ValueError('--channels belongs to decompress / decompress-dir: a preview is a way of reading a file')
        if getattr(flags, 'salvage', False):
            raise ValueError('--channels does not go with --salvage: a preview of a damaged file is not offered')
        if flags.channels < 1:
            raise ValueError('--channels {} is not at least 1'.format(flags.channels))
    if getattr(flags, 'region', None) is not None:
        if flags.command not in ('decompress', 'measure'):
            raise ValueError('--region belongs to decompress: a rectangle is in the pixels of one image')
        for name, why in (('salvage', 'region decode of a damaged file is not offered'),
                          ('partial', 'region decode of a cut file is not offered'),
                          ('recover', 'region decode of a damaged or cut file is not offered')):
            if getattr(flags, name, False):
                raise ValueError('--region does not go with --{}: {}'.format(name, why))
        region = parse_roi_arg(flags.region, '--region')
        if flags.command == 'measure' and min(region[2:]) < MIN_MEASURE_SIDE:
            raise ValueError('--region {!r}: MS-SSIM needs at least {} pixels a side'.format(flags.region, MIN_MEASURE_SIDE))
    if getattr(flags, 'checked', False):
        if flags.command not in WRITING_COMMANDS:
            raise ValueError('--checked belongs to compress / compress-dir: a file says by itself what it is')
        if flags.tile is None:
            raise ValueError('--checked needs --tile: the checksums of format 4 are per tile')
    if getattr(flags, 'wavefront', False):
        if flags.command not in WRITING_COMMANDS:
            raise ValueError('--wavefront belongs to compress / compress-dir: a file says by itself what it is')
        if flags.tile is None:
            raise ValueError('--wavefront needs --tile: format 5 codes every tile front by front')
    if getattr(flags, 'salvage', False) and flags.command not in ('decompress', 'decompress-dir') + TRANSCODE_COMMANDS:
        raise ValueError('--salvage belongs to decompress / decompress-dir')
    layers, progressive = getattr(flags, 'layers', None), getattr(flags, 'progressive', False)
    if layers is not None or progressive:
        name = '--layers' if layers is not None else '--progressive'
        if flags.command not in WRITING_COMMANDS:
            raise ValueError('{} belongs to compress / compress-dir: a file says by itself what it is'.format(name))
        if flags.tile is None:
            raise ValueError('{} needs --tile: format 6 cuts every tile into layers'.format(name))
        if getattr(flags, 'wavefront', False):
            raise ValueError('{} does not go with --wavefront: a layer is no prefix of a wavefront-ordered stream'.format(name))
        if layers is not None and progressive:
            raise ValueError('--layers does not go with --progressive: the one names the layer ends, the other takes the default ones')
        if layers is not None:
            parse_layers_arg(layers)
    front_layers, front_progressive = getattr(flags, 'front_layers', None), getattr(flags, 'front_progressive', False)
    if front_layers is not None or front_progressive:
        name = '--front-layers' if front_layers is not None else '--front-progressive'
        if flags.command not in WRITING_COMMANDS:
            raise ValueError('{} belongs to compress / compress-dir: a file says by itself what it is'.format(name))
        if flags.tile is None:
            raise ValueError('{} needs --tile: format 8 cuts every tile into layers'.format(name))
        if getattr(flags, 'wavefront', False):
            raise ValueError('{} does not go with --wavefront: format 8 implies the wavefront order, --wavefront writes the unlayered '
                             'format 5'.format(name))
        if layers is not None or progressive:
            raise ValueError('{} does not go with {}: the one cuts the wavefront order at fronts (format 8), the other the raster order '
                             'at channel planes (format 6)'.format(name, '--layers' if layers is not None else '--progressive'))
        if front_layers is not None and front_progressive:
            raise ValueError('--front-layers does not go with --front-progressive: the one names the layer ends, the other takes the '
                             'default ones')
        if front_layers is not None:
            parse_layers_arg(front_layers, '--front-layers')
    depth, depth_block = getattr(flags, 'depth', False), getattr(flags, 'depth_block', None)
    if depth_block is not None and not depth:
        raise ValueError('--depth-block needs --depth: it is the block side of the depth planes of format 10')
    if depth:
        if flags.command not in WRITING_COMMANDS:
            raise ValueError('--depth belongs to compress / compress-dir: a file says by itself what it is')
        if flags.tile is None:
            raise ValueError('--depth needs --tile: format 10 stores a depth plane per tile')
        if getattr(flags, 'wavefront', False):
            raise ValueError('--depth does not go with --wavefront: format 10 implies the wavefront order, --wavefront writes format 5, '
                             'which codes every position')
        for name, on in (('--layers', layers is not None), ('--progressive', progressive), ('--front-layers', front_layers is not None),
                         ('--front-progressive', front_progressive)):
            if on:
                raise ValueError('--depth does not go with {}: format 10 is one coder run per tile, the layered formats 6 and 8 cut a '
                                 'tile into several'.format(name))
        if depth_block is not None and not 1 <= depth_block <= 255:
            raise ValueError('--depth-block {} is not in 1 .. 255'.format(depth_block))
    rans, lanes = getattr(flags, 'rans', False), getattr(flags, 'lanes', None)
    if lanes is not None and not rans:
        raise ValueError('--lanes needs --rans: it is the number of interleaved coders of format 12')
    if rans:
        if flags.command not in WRITING_COMMANDS:
            raise ValueError('--rans belongs to compress / compress-dir: a file says by itself what it is')
        if flags.tile is None:
            raise ValueError('--rans needs --tile: format 12 codes every tile with W interleaved coders')
        if getattr(flags, 'checked', False):
            raise ValueError('--rans does not go with --checked: format 12 has its own CRC per tile, --checked writes format 4')
        if getattr(flags, 'wavefront', False):
            raise ValueError('--rans does not go with --wavefront: format 12 implies the wavefront order, --wavefront writes format 5, '
                             'one arithmetic coder per tile')
        if depth:
            raise ValueError('--rans does not go with --depth: format 10 leaves positions out of an arithmetic coder\'s stream, format '
                             '12 codes every position with W rANS coders')
        for name, on in (('--layers', layers is not None), ('--progressive', progressive), ('--front-layers', front_layers is not None),
                         ('--front-progressive', front_progressive)):
            if on:
                raise ValueError('--rans does not go with {}: format 12 is one interleaved stream per tile, the layered formats 6 and 8 '
                                 'cut a tile into several'.format(name))
        if lanes is not None and lanes not in RANS_LANES:
            raise ValueError('--lanes {} is not one of {}'.format(lanes, ', '.join(str(w) for w in RANS_LANES)))
    if getattr(flags, 'partial', False):
        if flags.command not in ('decompress', 'decompress-dir'):
            raise ValueError('--partial belongs to decompress / decompress-dir: it reads a prefix of a layered file')
        if getattr(flags, 'salvage', False):
            raise ValueError('--partial does not go with --salvage: salvage of layered files is not offered')
        if getattr(flags, 'channels', None) is not None:
            raise ValueError('--partial does not go with --channels: the complete layers decide the channels')
    if getattr(flags, 'recover', False):
        if flags.command not in ('decompress', 'decompress-dir') + TRANSCODE_COMMANDS:
            raise ValueError('--recover belongs to decompress / decompress-dir: it reads what a damaged or cut layered file still holds')
        if getattr(flags, 'salvage', False):
            raise ValueError('--recover does not go with --salvage: the one reads layered files (format 6), the other formats 4 and 5')
        if getattr(flags, 'partial', False):
            raise ValueError('--recover does not go with --partial: the one reads every tile as far as it goes, the other the layers '
                             'that are complete in all tiles')
        if getattr(flags, 'channels', None) is not None:
            raise ValueError('--recover does not go with --channels: what every tile still holds decides its channels')


def parse_roi_arg(text, option='--roi'):
    """'X,Y,W,H' -> (x, y, w, h); a ValueError for anything but four integers with a positive extent (the image is checked by cap_plane)"""
    try:
        x, y, w, h = (int(v) for v in str(text).split(','))
    except ValueError:
        raise ValueError('{} {!r} is not X,Y,W,H in pixels'.format(option, text))
    if w < 1 or h < 1:
        raise ValueError('{} {!r}: the extent {} x {} is not positive'.format(option, text, w, h))
    return x, y, w, h


def _budget_of(flags, H, W):
    """--max-bytes, or --bpp over the H x W pixels of one image, or None"""
    if getattr(flags, 'max_bytes', None) is not None:
        return int(flags.max_bytes)
    if getattr(flags, 'bpp', None) is not None:
        return int(flags.bpp * H * W // 8)
    return None


def _rdo_note(lam, changed, count):
    return ', lambda {:g}: {} of {} symbols differ from the quantiser\'s'.format(lam, changed, count)


def _budget_note(level, probes):
    return ', cap level {:g} after {} codings'.format(level, probes)


def _quality_of(flags):
    """--min-psnr / --min-ms-ssim as the keyword arguments of compress_to_quality / transcode_to_quality, or None"""
    if getattr(flags, 'min_psnr', None) is not None:
        return {'psnr': flags.min_psnr}
    if getattr(flags, 'min_ms_ssim', None) is not None:
        return {'ms_ssim': flags.min_ms_ssim}
    return None


def _measure_text(m):
    return 'PSNR {:.4f} dB, MS-SSIM {:.6f}, MSE {:.4f}'.format(m.psnr, m.ms_ssim, m.mse)


def _quality_note(level, measure, probes):
    return ', cap level {:g} after {} probes: {}'.format(level, probes, _measure_text(measure))


def _measure_line(path, m, channels=None, C=None, rect=None):
    line = '{}: {} bytes = {:.4f} bpp, {}'.format(path, m.bytes, m.bpp, _measure_text(m))
    if rect is not None:
        line += ', of the region x {}..{} y {}..{}'.format(rect[0], rect[2], rect[1], rect[3])
    return line if channels is None else '{}, preview from {} of {} channels'.format(line, channels, C)


def _rd_line(level, m, key='level'):
    return '{} {:g}: {} bytes = {:.4f} bpp, {}'.format(key, level, m.bytes, m.bpp, _measure_text(m))


def rd_table(codec, rows, image, H, W, rois=None, key='level'):
    """what the rd command writes as JSON: the rows of Codec.rd_curve -- or, with key='rdo', of Codec.rdo_curve, a lambda per row in
    place of a cap level -- with the format and the configs they were measured under"""
    return {'image': image, 'H': int(H), 'W': int(W), 'ae_config': codec.ae_name, 'pc_config': codec.pc_name,
            'format': codec.written_version(), 'tile': None if codec.tile is None else [v * codec.factor for v in codec.tile],
            'rois': [list(r) for r in rois or []],
            'rows': [dict(m._asdict(), **{key: level}) for level, m in rows]}


def parse_rdo_levels_arg(text, option='--rdo-levels'):
    """'0,0.01,0.1' -> [0.0, 0.01, 0.1]; a ValueError for anything but comma-separated numbers with 0 <= lambda < inf"""
    try:
        lams = [float(v) for v in str(text).split(',')]
    except ValueError:
        raise ValueError('{} {!r} is not a comma-separated list of numbers'.format(option, text))
    if not lams or not all(0.0 <= v < float('inf') for v in lams):
        raise ValueError('{} {!r}: every lambda is a number with 0 <= lambda < inf'.format(option, text))
    return lams


def parse_layers_arg(text, option='--layers'):
    """'4,8,16,32' -> [4, 8, 16, 32]; a ValueError for anything but comma-separated positive integers (C is checked by the codec)"""
    try:
        ends = [int(v) for v in str(text).split(',')]
    except ValueError:
        raise ValueError('{} {!r} is not a comma-separated list of integers'.format(option, text))
    if not 1 <= len(ends) <= MAX_LAYERS or ends[0] < 1 or any(b <= a for a, b in zip(ends, ends[1:])):
        raise ValueError('{} {!r}: 1 to {} increasing layer ends from at least 1, the last one C'.format(option, text, MAX_LAYERS))
    return ends


def _layers_option(flags, C):
    """the `layers` argument of Codec for a command line, --layers checked against the C of the autoencoder's config: decided
    before any model is built"""
    if getattr(flags, 'layers', None) is not None:
        return check_layer_ends(parse_layers_arg(flags.layers), C)
    return 'default' if getattr(flags, 'progressive', False) else None


def _depth_option(flags):
    """the `depth_block` argument of Codec for a command line: None without --depth, else --depth-block or its default"""
    if not getattr(flags, 'depth', False):
        return None
    return DEFAULT_DEPTH_BLOCK if getattr(flags, 'depth_block', None) is None else int(flags.depth_block)


def _rans_option(flags):
    """the `rans` argument of Codec for a command line: None without --rans, else --lanes or 'default'"""
    if not getattr(flags, 'rans', False):
        return None
    return 'default' if getattr(flags, 'lanes', None) is None else int(flags.lanes)


def _front_layers_option(flags, C):
    """the `front_layers` argument of Codec for a command line, as _layers_option"""
    if getattr(flags, 'front_layers', None) is not None:
        return check_layer_ends(parse_layers_arg(flags.front_layers, '--front-layers'), C)
    return 'default' if getattr(flags, 'front_progressive', False) else None


def check_dir_args(flags, factor):
    """everything about a -dir command line that can be refused without a device -> (jobs, tile or None)"""
    check_option_args(flags)
    if flags.batch < 1:
        raise ValueError('--batch {} is not at least 1'.format(flags.batch))
    tile = None
    if flags.tile is not None:
        if flags.command not in ('compress-dir', 'transcode-dir'):
            raise ValueError('--tile belongs to compress / compress-dir: a file says by itself how it is tiled')
        if flags.tile <= 0 or flags.tile % factor != 0:
            raise ValueError('--tile {} is not a positive multiple of the subsampling factor {}'.format(flags.tile, factor))
        tile = (flags.tile // factor, flags.tile // factor)
    jobs = list_dir_jobs(flags.input, flags.output, flags.command)
    if os.path.exists(flags.output) and not os.path.isdir(flags.output):
        raise ValueError('{}: output {!r} exists and is not a directory'.format(flags.command, flags.output))
    return jobs, tile


def _main_dir(flags, ae_config, pc_config):
    """compress-dir / decompress-dir: one model build, --batch files per compress_many / decompress_many call"""
    from PIL import Image
    from . import autoencoder, val, weights as _weights
    jobs, tile = check_dir_args(flags, int(autoencoder.get_network_cls(ae_config).get_subsampling_factor()))
    layers = _layers_option(flags, ae_config.num_chan_bn) if tile is not None else None
    front_layers = _front_layers_option(flags, ae_config.num_chan_bn) if tile is not None else None
    if flags.weights == 'synthetic':
        wts = _weights.synthetic_weights(ae_config, pc_config, seed=flags.synthetic_seed)
    else:
        wts = val.load_weights_for_job(None, flags.weights, ae_config, pc_config)
    codec = Codec(ae_config, pc_config, wts, flags.device, tile=tile, checked=flags.checked,
                  order='wavefront' if flags.wavefront and tile is not None else 'raster',
                  layers=layers, front_layers=front_layers, depth_block=_depth_option(flags) if tile is not None else None,
                  rans=_rans_option(flags) if tile is not None else None)
    channels = check_channels(getattr(flags, 'channels', None), codec.C)
    os.makedirs(flags.output, exist_ok=True)
    total_in = total_out = total_pixels = 0
    if flags.command == 'transcode-dir':
        return _transcode_dir(flags, codec, jobs)
    if flags.command == 'decompress-dir' and flags.salvage:
        return _salvage_dir(flags, codec, jobs)
    if flags.command == 'decompress-dir' and flags.partial:
        return _partial_dir(codec, jobs)
    if flags.command == 'decompress-dir' and getattr(flags, 'recover', False):
        return _recover_dir(flags, codec, jobs)
    for start in range(0, len(jobs), flags.batch):
        part = jobs[start:start + flags.batch]
        if flags.command == 'compress-dir':
            imgs = [np.asarray(Image.open(src).convert('RGB'), dtype=np.uint8) for src, _ in part]     # as compress_file reads them
            notes = [''] * len(imgs)
            if _budget_of(flags, 1, 1) is not None:              # a budget per file: a search per file, one after the other
                found = [codec.compress_to_budget(img, _budget_of(flags, img.shape[0], img.shape[1])) for img in imgs]
                datas, notes = [d for d, _, _ in found], [_budget_note(level, probes) for _, level, probes in found]
            elif _quality_of(flags) is not None:                 # a target per file, likewise
                found = [codec.compress_to_quality(img, **_quality_of(flags)) for img in imgs]
                datas, notes = [d for d, _, _, _ in found], [_quality_note(level, m, probes) for _, level, m, probes in found]
            else:
                datas = codec.compress_many(imgs, caps=None if getattr(flags, 'cap', None) is None else [flags.cap] * len(imgs),
                                            rdos=None if getattr(flags, 'rdo', None) is None else [flags.rdo] * len(imgs))
            for (src, dst), img, data, note in zip(part, imgs, datas, notes):
                with open(dst, 'wb') as f:
                    f.write(data)
                print(_compress_line(dst, data, img.shape[0] * img.shape[1]) + note)
                total_in, total_out, total_pixels = total_in + os.path.getsize(src), total_out + len(data), total_pixels + img.shape[0] * img.shape[1]
        else:
            datas = []
            for src, _ in part:
                with open(src, 'rb') as f:
                    datas.append(f.read())
            try:
                imgs = codec.decompress_many(datas, channels=channels)
            except ValueError as e:
                m = re.match(r'file (\d+): ', str(e))
                raise ValueError('{}: {}'.format(part[int(m.group(1))][0], str(e)[m.end():]) if m else str(e))
            for (src, dst), data, img in zip(part, datas, imgs):
                Image.fromarray(img).save(dst)
                print(_decompress_line(dst, img, len(data), channels, codec.C))
                total_in, total_out, total_pixels = total_in + len(data), total_out + os.path.getsize(dst), total_pixels + img.shape[0] * img.shape[1]
    if flags.command == 'compress-dir':
        print('total: {} files, {} pixels, {} bytes = {:.4f} bpp'.format(len(jobs), total_pixels, total_out, 8.0 * total_out / total_pixels))
    else:
        print('total: {} files, {} pixels from {} bytes = {:.4f} bpp'.format(len(jobs), total_pixels, total_in, 8.0 * total_in / total_pixels))
    return 0


def _source_version(data):
    """the format version a file names, before anything else of it is looked at (the readers decide what it is worth); None without one"""
    return struct.unpack('<H', data[4:6])[0] if len(data) >= 6 and data[:4] == MAGIC else None


def _transcode_line(path, data, out):
    return '{}: format {} -> format {}, {} -> {} bytes'.format(path, _source_version(data), _source_version(out), len(data), len(out))


def _cap_option(value):
    """--cap / --background of a transcode (check_option_args has seen it: an integer or +inf) -> what Codec.transcode takes"""
    return None if value is None else value if value == float('inf') else int(value)


def _transcode_one(flags, codec, src, dst, data, rois=None):
    """one file of transcode / transcode-dir by the flags' own path -- repair, budget or plain -- written and printed"""
    report = None
    note = ''
    if getattr(flags, 'salvage', False) or getattr(flags, 'recover', False):
        try:
            out = codec.transcode(data, cap=_cap_option(flags.cap))
        except ValueError:                                           # (as decompress --salvage: the strict reader first)
            out, report = codec.repair(data, cap=_cap_option(flags.cap))
    elif flags.max_bytes is not None or flags.bpp is not None:
        c = parse_container(data)
        out, level, probes = codec.transcode_to_budget(data, _budget_of(flags, c.H, c.W), rois=rois or None)
        note = _budget_note(level, probes)
    elif _quality_of(flags) is not None:
        out, level, m, probes = codec.transcode_to_quality(data, **_quality_of(flags))
        note = _quality_note(level, m, probes)
    else:
        out = codec.transcode(data, cap=_cap_option(flags.cap), rois=rois or None, background=_cap_option(flags.background))
    with open(dst, 'wb') as f:
        f.write(out)
    print(_transcode_line(dst, data, out) + note)
    if isinstance(report, SalvageReport) and (report.damaged or not report.file_crc_ok):
        print(_damage_line(src, report))
    if isinstance(report, RecoverReport):
        print(_recover_line(src, report))
    return out


def _transcode_dir(flags, codec, jobs):
    """transcode-dir: --batch files per transcode_many call; with a budget or a quality target a search per file, with --salvage / --recover a repair per
    file, and there a file of which nothing can be read is named on stderr and skipped.  Exit status 0 when every file was written."""
    written = total_in = total_out = 0
    one_by_one = flags.salvage or flags.recover or _budget_of(flags, 1, 1) is not None or _quality_of(flags) is not None
    for start in range(0, len(jobs), flags.batch):
        part = jobs[start:start + flags.batch]
        datas = []
        for src, _ in part:
            with open(src, 'rb') as f:
                datas.append(f.read())
        if one_by_one:
            for (src, dst), data in zip(part, datas):
                try:
                    out = _transcode_one(flags, codec, src, dst, data)
                except ValueError as e:
                    if not (flags.salvage or flags.recover):
                        raise ValueError('{}: {}'.format(src, e))
                    print('error: {}: {}'.format(src, e), file=sys.stderr)
                    continue
                written, total_in, total_out = written + 1, total_in + len(data), total_out + len(out)
            continue
        try:
            outs = codec.transcode_many(datas, caps=None if flags.cap is None else [_cap_option(flags.cap)] * len(datas))
        except ValueError as e:
            m = re.match(r'file (\d+): ', str(e))
            raise ValueError('{}: {}'.format(part[int(m.group(1))][0], str(e)[m.end():]) if m else str(e))
        for (src, dst), data, out in zip(part, datas, outs):
            with open(dst, 'wb') as f:
                f.write(out)
            print(_transcode_line(dst, data, out))
            written, total_in, total_out = written + 1, total_in + len(data), total_out + len(out)
    print('total: {} of {} files, {} -> {} bytes'.format(written, len(jobs), total_in, total_out))
    return 0 if written == len(jobs) else 2


def _partial_line(path, report):
    return '{}: layers decoded {} of {}: {} channels{}'.format(path, report.layers_decoded, report.layers_total, report.channels,
                                                             '' if report.file_crc_ok else ', the CRC over the file is missing or wrong')


def _partial_dir(codec, jobs):
    """decompress-dir --partial: every file through decompress_partial; a file of which nothing can be decoded is named on stderr
    and skipped.  Exit status 0 when every file gave an image, else 2."""
    from PIL import Image
    written = 0
    for src, dst in jobs:
        with open(src, 'rb') as f:
            data = f.read()
        try:
            img, report = codec.decompress_partial(data)
        except ValueError as e:
            print('error: {}: {}'.format(src, e), file=sys.stderr)
            continue
        Image.fromarray(img).save(dst)
        print(_decompress_line(dst, img, len(data)))
        print(_partial_line(src, report))
        written += 1
    print('total: {} of {} files'.format(written, len(jobs)))
    return 0 if written == len(jobs) else 2


def _recover_dir(flags, codec, jobs):
    """decompress-dir --recover: --batch files per recover_many call; a file of which nothing can be read is named on stderr and
    skipped.  Exit status 0 when every file gave an image, else 2."""
    from PIL import Image
    written = 0
    for start in range(0, len(jobs), flags.batch):
        part = jobs[start:start + flags.batch]
        datas = []
        for src, _ in part:
            with open(src, 'rb') as f:
                datas.append(f.read())
        try:
            results = codec.recover_many(datas)
        except ValueError:
            results = []                                   # one of them cannot be read: find out which
            for (src, _), data in zip(part, datas):
                try:
                    results.append(codec.recover(data))
                except ValueError as e:
                    print('error: {}: {}'.format(src, e), file=sys.stderr)
                    results.append(None)
        for (src, dst), data, res in zip(part, datas, results):
            if res is None:
                continue
            Image.fromarray(res[0]).save(dst)
            print(_decompress_line(dst, res[0], len(data)))
            print(_recover_line(src, res[1]))
            written += 1
    print('total: {} of {} files'.format(written, len(jobs)))
    return 0 if written == len(jobs) else 2


def _salvage_dir(flags, codec, jobs):
    """decompress-dir --salvage: strict for the files that pass (any format), salvage for the others; a file of which nothing can be
    recovered is named on stderr and skipped.  Exit status 0 when every file gave an image, else 2."""
    from PIL import Image
    total_in = total_pixels = written = 0
    for start in range(0, len(jobs), flags.batch):
        part = jobs[start:start + flags.batch]
        datas, good = [], []
        for src, _ in part:
            with open(src, 'rb') as f:
                datas.append(f.read())
        results = [None] * len(part)
        for i, data in enumerate(datas):
            try:
                parse_container(data)
                good.append(i)
            except ValueError:
                pass
        try:
            for i, img in zip(good, codec.decompress_many([datas[i] for i in good])):
                results[i] = (img, None)
        except ValueError:
            good = []                                      # (another model, a decoder status: file by file below)
        rest = [i for i in range(len(part)) if results[i] is None]
        try:
            for i, r in zip(rest, codec.salvage_many([datas[i] for i in rest])):
                results[i] = r
        except ValueError:
            for i in rest:                                 # one of them cannot be recovered: find out which
                try:
                    results[i] = (codec.decompress(datas[i]), None)
                except ValueError:
                    try:
                        results[i] = codec.salvage(datas[i])
                    except ValueError as e:
                        print('error: {}: {}'.format(part[i][0], e), file=sys.stderr)
        for (src, dst), data, res in zip(part, datas, results):
            if res is None:
                continue
            img, report = res
            Image.fromarray(img).save(dst)
            print(_decompress_line(dst, img, len(data)))
            if report is not None and (report.damaged or not report.file_crc_ok):
                print(_damage_line(src, report))
            written, total_in, total_pixels = written + 1, total_in + len(data), total_pixels + img.shape[0] * img.shape[1]
    print('total: {} of {} files, {} pixels from {} bytes'.format(written, len(jobs), total_pixels, total_in))
    return 0 if written == len(jobs) else 2


def list_verify_files(paths):
    """verify's arguments -> the files it checks: a file as it is, a directory's *.icf sorted by name"""
    files = []
    for path in paths:
        if os.path.isdir(path):
            files += [os.path.join(path, n) for n in sorted(os.listdir(path))
                      if n.lower().endswith('.icf') and os.path.isfile(os.path.join(path, n))]
        else:
            files.append(path)
    return files


def verify_file(data):
    """container bytes -> (ok, text).  The strict reader decides; for a format-4 file that it refuses, the salvage reader names
    the damaged tiles.  Host only: no model, no device."""
    try:
        c = parse_container(data)
        if isinstance(c, LayeredContainer):
            G = len(c.layer_ends)
            return True, 'ok (format {}, {} bytes, G = {} layers, ends {}, prefix lengths {})'.format(
                c.version, len(data), G, ','.join(str(e) for e in c.layer_ends), ','.join(str(layer_prefix_bytes(c, g)) for g in range(G + 1)))
        if isinstance(c, DepthContainer):
            return True, 'ok (format {}, {} bytes, depth blocks of {} cells)'.format(c.version, len(data), c.depth_block)
        if isinstance(c, RansContainer):
            return True, 'ok (format {}, {} bytes, W = {} coders per tile)'.format(c.version, len(data), c.lanes)
        return True, 'ok (format {}, {} bytes)'.format(c.version, len(data))
    except ValueError as strict:
        if _source_version(data) in _LAYERED_VERSIONS:
            try:
                c, complete, _ = parse_partial(data)
            except ValueError as e:
                return False, str(e)
            return False, '{} of {} layers complete, but {}'.format(complete, len(c.layer_ends), strict)
        try:
            c, damage, file_crc_ok = parse_salvage(data)
        except ValueError as e:
            if _source_version(data) in _WITH_CRCS:
                return False, str(e)
            return False, str(strict)
        if not damage:
            return False, 'all {} tiles intact, but {}'.format(len(c.streams), strict)
        return False, '{} of {} tiles damaged: {}'.format(len(damage), len(c.streams), ', '.join(
            'tile {} ({})'.format(t, why) for t, why in damage))


def _main_verify(argv):
    p = argparse.ArgumentParser(prog='codec verify', description='check codec files on the host: no model, no device')
    p.add_argument('paths', nargs='+', metavar='PATH', help='a codec file, or a directory whose *.icf files are checked')
    flags = p.parse_args(argv)
    bad = 0
    files = list_verify_files(flags.paths)
    for path in files:
        try:
            with open(path, 'rb') as f:
                ok, text = verify_file(f.read())
        except (IOError, OSError) as e:
            ok, text = False, 'cannot read: {}'.format(e)
        bad += not ok
        print('{}: {}'.format(path, text))
    if not files:
        print('verify: no file to check', file=sys.stderr)
        return 1
    return 1 if bad else 0


INFO_FACTOR = 8                                                      # the subsampling factor of the one architecture (info builds no network to ask)


def _tile_bytes(c):
    """coded bytes per tile of a parsed tiled container, all layers of a layered one"""
    return [sum(len(s) for s in b) if isinstance(c, LayeredContainer) else len(b) for b in c.streams]


def _region_line(path, img, plan, channels=None, C=None):
    y0, x0, wh, ww = plan.window
    line = '{}: {} x {} at ({}, {}), from {} tiles: rows {} .. {}, columns {} .. {}, a window of {} x {} cells'.format(
        path, img.shape[0], img.shape[1], plan.rect[1], plan.rect[0], len(plan.tiles), plan.rows[0], plan.rows[1] - 1,
        plan.cols[0], plan.cols[1] - 1, wh, ww)
    return line if channels is None else '{}, preview from {} of {} channels'.format(line, channels, C)


def info_file(data, region=None):
    """container bytes -> the text of `info`: format, image size, latent and tile extents, the tile grid, layer ends, bytes per tile
    and per layer; with region = (x, y, w, h) the tiles and the window decompress_region would decode for it and their share of
    the payload (region_plan at the reach of the file's autoencoder config, an even first cell as Codec.region_plan asks; once for
    the arithmetic's reach and once for the F(4x4) kernels', since which of them a picture's decoder runs is the library's decision).  The
    strict reader parses the file; host only: no model, no device.  A ValueError for a file the reader refuses, a format-1 file with
    a region, a config that is not found."""
    c = parse_container(data)
    lines = ['format {}, {} bytes, model {} / {} ({:08x})'.format(c.version, len(data), c.ae_name, c.pc_name, c.fingerprint),
             'image {} x {} (H x W), latent {} x {} x {} (C x h x w)'.format(c.H, c.W, c.C, c.h, c.w)]
    if not isinstance(c, _TILED):
        lines.append('one stream over the whole volume, {} bytes: no tiles'.format(len(c.payload)))
        if region is not None:
            raise ValueError('region decode needs tiles: a format-{} file is one stream over the whole volume and decodes only as a '
                             'whole; write it with --tile'.format(c.version))
        return '\n'.join(lines)
    per_tile = _tile_bytes(c)
    rows, cols = (c.h + c.th - 1) // c.th, (c.w + c.tw - 1) // c.tw
    lines.append('tiles of {} x {} cells, grid {} x {} = {} tiles, last row {} cells high, last column {} wide'.format(
        c.th, c.tw, rows, cols, len(per_tile), c.h - (rows - 1) * c.th, c.w - (cols - 1) * c.tw))
    lines.append('payload {} bytes; per tile min {}, mean {:.1f}, max {}'.format(sum(per_tile), min(per_tile), sum(per_tile) / float(len(per_tile)), max(per_tile)))
    lines.append('bytes per tile: {}'.format(','.join(str(n) for n in per_tile)))
    if isinstance(c, LayeredContainer):
        lines.append('layer ends {}; bytes per layer {}'.format(','.join(str(e) for e in c.layer_ends),
                                                                ','.join(str(sum(len(s) for s in layer)) for layer in c.segments)))
    if isinstance(c, DepthContainer):
        live, steps, plane_bytes = 0, [], 0
        for (_, _, a, b), s in zip(tile_grid(c.h, c.w, c.th, c.tw), c.streams):
            depth, _ = split_depth_stream(s, c.C, a, b, c.depth_block)
            live += int(depth_live(c.C, a, b, depth, c.depth_block).sum())
            steps.append(depth_front_steps(a, b, int(depth.max())))
            plane_bytes += depth.size
        lines.append('depth blocks of {} x {} cells, {} bytes of depth planes; live share {:.4f} ({} of {} positions are coded)'.format(
            c.depth_block, c.depth_block, plane_bytes, live / float(c.C * c.h * c.w), live, c.C * c.h * c.w))
        lines.append('front steps per tile: {} (all {} channels: {})'.format(
            ','.join(str(n) for n in steps), c.C, ','.join(str(depth_front_steps(a, b, c.C)) for _, _, a, b in tile_grid(c.h, c.w, c.th, c.tw))))
    if isinstance(c, RansContainer):
        state_bytes = 4 * c.lanes * len(per_tile)
        lines.append('W = {} interleaved coders per tile, {} bytes of coder states: {:.4f} of the payload'.format(
            c.lanes, state_bytes, state_bytes / float(max(1, sum(per_tile)))))
    if region is not None:
        from . import config_parser
        ae_config, _ = config_parser.parse(_resolve_config(c.ae_name, 'ae_configs', 'CONFIG_BASE_AE'))
        before, after = decoder_reach(ae_config.arch_param_B)
        f = INFO_FACTOR
        if (c.h, c.w) != ((c.H + f - 1) // f, (c.W + f - 1) // f):
            raise ValueError('header mismatch: symbol volume {} x {} does not belong to a {} x {} image (expected {} x {})'.format(
                c.h, c.w, c.H, c.W, (c.H + f - 1) // f, (c.W + f - 1) // f))
        B = int(ae_config.arch_param_B)
        # which kernels a picture's decoder runs is the library's decision (Codec.region_plan asks it); both plans are shown
        for what, reach in (('reach {} before, {} after'.format(before, after), (before, after)),
                            ('where the decoder runs its F(4x4) kernels', lambda p0, p1: decoder_cells(p0, p1, B, True, True))):
            plan = region_plan(c.H, c.W, f, c.h, c.w, c.th, c.tw, region, reach, align=2)
            y0, x0, wh, ww = plan.window
            part = sum(per_tile[t] for t in plan.tiles)
            lines.append('region {},{},{},{} ({}): tile rows {} .. {}, columns {} .. {}, {} of {} tiles'.format(
                plan.rect[0], plan.rect[1], plan.rect[2], plan.rect[3], what, plan.rows[0], plan.rows[1] - 1, plan.cols[0],
                plan.cols[1] - 1, len(plan.tiles), len(per_tile)))
            lines.append('  window {} x {} cells at ({}, {}), a decoder pass of {} x {} pixels of {} x {}; {} of {} payload bytes = {:.1f} %'.format(
                wh, ww, y0, x0, wh * f, ww * f, c.h * f, c.w * f, part, sum(per_tile), 100.0 * part / max(1, sum(per_tile))))
            lines.append('  tiles {}'.format(','.join(str(t) for t in plan.tiles)))
    return '\n'.join(lines)


def _main_info(argv):
    p = argparse.ArgumentParser(prog='codec info', description='what a codec file holds, and what a region of it would decode: no model, no device')
    p.add_argument('paths', nargs='+', metavar='PATH', help='a codec file, or a directory whose *.icf files are described')
    p.add_argument('--region', default=None, metavar='X,Y,W,H', help='the tiles and the window decompress --region would decode for this rectangle')
    flags = p.parse_args(argv)
    try:
        region = None if flags.region is None else parse_roi_arg(flags.region, '--region')
    except ValueError as e:
        print('error: {}'.format(e), file=sys.stderr)
        return 2
    bad = 0
    files = list_verify_files(flags.paths)
    for path in files:
        try:
            with open(path, 'rb') as f:
                text = info_file(f.read(), region)
        except (IOError, OSError) as e:
            bad, text = bad + 1, 'cannot read: {}'.format(e)
        except ValueError as e:
            bad, text = bad + 1, str(e)
        print('{}: {}'.format(path, text.replace('\n', '\n  ')))
    if not files:
        print('info: no file to describe', file=sys.stderr)
        return 1
    return 1 if bad else 0


STREAM_CHUNK = 16384


def _main_stream(flags, codec):
    """stream: the file fed chunk by chunk, a picture and a recover line each time a tile has gained a layer"""
    from PIL import Image
    if os.path.exists(flags.output) and not os.path.isdir(flags.output):
        raise ValueError('stream: output {!r} exists and is not a directory'.format(flags.output))
    with open(flags.input, 'rb') as f:
        data = f.read()
    chunk = STREAM_CHUNK if flags.chunk is None else flags.chunk
    stem = os.path.splitext(os.path.basename(flags.input))[0]
    dec, shown = codec.open_stream(fronts=getattr(flags, 'fronts', False)), None
    for pos in range(0, len(data), chunk):
        if not dec.feed(data[pos:pos + chunk]):
            continue
        layers = dec.progress()
        if layers == shown or not any(layers):
            continue
        img, report = dec.image()
        shown = layers
        os.makedirs(flags.output, exist_ok=True)
        path = os.path.join(flags.output, '{}.{:09d}.png'.format(stem, dec.bytes_fed))
        Image.fromarray(img).save(path)
        print(_recover_line(path, report))
    if shown is None:
        raise ValueError('no complete layer: {} holds {} bytes and no tile\'s layer 0'.format(flags.input, len(data)))


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    if argv and argv[0] == 'verify':
        return _main_verify(argv[1:])
    if argv and argv[0] == 'info':
        return _main_info(argv[1:])
    p = argparse.ArgumentParser(description='compress an image to a codec file, or a codec file back to an image; transcode a codec '
                                            'file to another format or a lower rate without its image; '
                                            'the -dir commands do so for every file of a directory, --batch files per call')
    p.add_argument('command', choices=['compress', 'decompress', 'compress-dir', 'decompress-dir', 'stream', 'transcode', 'transcode-dir',
                                       'measure', 'rd'])
    p.add_argument('input')
    p.add_argument('output')
    p.add_argument('--ae_config', default='cvpr/low', help='a config file, or a name below $CONFIG_BASE_AE / the package\'s ae_configs')
    p.add_argument('--pc_config', default='cvpr/res_shallow', help='the same for the context model')
    p.add_argument('--weights', default='synthetic', help="'synthetic', an .npz of checkpoint variables, or a TF-1 checkpoint prefix / "
                                                          "ckpts dir (as val.py)")
    p.add_argument('--synthetic_seed', type=int, default=1234, help='seed of --weights synthetic')
    p.add_argument('--device', default='cuda:0')
    p.add_argument('--tile', type=int, default=None, metavar='PIXELS',
                   help='compress: square tiles of this many image pixels (a positive multiple of the subsampling factor), one stream '
                        'per tile, decoded concurrently (format 2); default: one stream (format 1)')
    p.add_argument('--batch', type=int, default=8, metavar='N', help='the -dir commands: files per call (default 8)')
    p.add_argument('--checked', action='store_true', help='compress / compress-dir with --tile: a CRC per tile stream and one over the '
                                                          'header (format 4), so that a damaged file can be salvaged')
    p.add_argument('--wavefront', action='store_true', help='compress / compress-dir with --tile: the layout of --checked, every tile coded '
                                                            'front by front (format 5), which decodes a front at a time')
    p.add_argument('--layers', default=None, metavar='a,b,..',
                   help='compress / compress-dir with --tile: layered tiles (format 6) with these layer ends, increasing, the last one C: '
                        'a prefix of the file decodes as a preview; not with --wavefront')
    p.add_argument('--progressive', action='store_true', help='compress / compress-dir with --tile: --layers with the default ends C/8, C/4, C/2, C')
    p.add_argument('--front-layers', dest='front_layers', default=None, metavar='a,b,..',
                   help='compress / compress-dir with --tile: front-layered tiles (format 8) with these layer ends: every tile coded front by '
                        'front as with --wavefront and cut at fronts, so that a prefix of the file decodes as a preview, a front at a time; '
                        'not with --wavefront, --layers or --progressive')
    p.add_argument('--front-progressive', dest='front_progressive', action='store_true',
                   help='compress / compress-dir with --tile: --front-layers with the default ends C/8, C/4, C/2, C')
    p.add_argument('--depth', action='store_true',
                   help='compress / compress-dir with --tile: depth-mapped tiles (format 10): the layout of --wavefront plus a depth plane per '
                        'tile, and the positions above a block\'s depth -- which hold the fill symbol -- are neither coded nor decoded; '
                        'not with --wavefront or the layered formats')
    p.add_argument('--depth-block', dest='depth_block', type=int, default=None, metavar='B',
                   help='--depth: blocks of B x B latent cells, 1 .. 255 (default {})'.format(DEFAULT_DEPTH_BLOCK))
    p.add_argument('--rans', action='store_true',
                   help='compress / compress-dir with --tile: lane-parallel rANS tiles (format 12): the order of --wavefront, every tile coded '
                        'by W interleaved rANS coders that the decoder steps a round at a time; not with --checked, --wavefront, --depth '
                        'or the layered formats')
    p.add_argument('--lanes', type=int, default=None, metavar='W',
                   help='--rans: the number of coders per tile, one of {} (default {})'.format(', '.join(str(w) for w in RANS_LANES),
                                                                                               DEFAULT_RANS_LANES))
    p.add_argument('--partial', action='store_true', help='decompress / decompress-dir: decode the complete layers of a (cut) format-6 / format-8 file and '
                                                          'print how many of them; not with --salvage or --channels')
    p.add_argument('--recover', action='store_true', help='decompress / decompress-dir: read what a damaged or cut format-6 file still holds, every '
                                                          'tile up to its own intact leading layers, the rest filled from the neighbours '
                                                          'that hold it; names the incomplete tiles; not with --salvage, --partial or --channels')
    p.add_argument('--salvage', action='store_true', help='decompress / decompress-dir: read what a damaged format-4 / format-5 file still holds; '
                                                          'damaged tiles are filled from their neighbours and named')
    p.add_argument('--channels', type=int, default=None, metavar='K',
                   help='decompress / decompress-dir: a preview from the first K latent channels only (any format; the decoder stops '
                        'after them, the other channels get the centre nearest zero); not with --salvage')
    p.add_argument('--chunk', type=int, default=None, metavar='BYTES',
                   help='stream: feed the file in pieces of this many bytes (default {})'.format(STREAM_CHUNK))
    p.add_argument('--fronts', action='store_true', help='stream: take a front-layered file (format 8) as well, every front of every tile '
                                                         'swept once; without it such a file is refused')
    p.add_argument('--cap', type=float, default=None, metavar='T',
                   help='compress / compress-dir: an upper bound T in [0, C] on the importance map, the same in every latent cell: a rate '
                        'below the model\'s own (0: every channel masked; C or more: no cap); the file format is unchanged; '
                        'transcode / transcode-dir: the same on a file\'s symbols, an integer level K only')
    p.add_argument('--roi', action='append', default=None, metavar='X,Y,W,H',
                   help='compress: a rectangle in image pixels that keeps --cap (or no cap) while the rest gets --background; repeatable')
    p.add_argument('--background', type=float, default=None, metavar='T', help='compress / transcode with --roi: the cap outside the rectangles')
    p.add_argument('--max-bytes', dest='max_bytes', type=int, default=None, metavar='N',
                   help='compress / compress-dir: the largest cap level (of the grid k C / 256) whose file has at most N bytes; with --roi '
                        'the rectangles stay uncapped and the level is the background\'s; prints the level and the number of codings; '
                        'transcode / transcode-dir: the largest integer level 0 .. C')
    p.add_argument('--bpp', type=float, default=None, metavar='B', help='compress / compress-dir: --max-bytes floor(B H W / 8), per image')
    p.add_argument('--region', default=None, metavar='X,Y,W,H',
                   help='decompress: only this rectangle of the image, in image pixels (clipped to it), decoded from the tiles it needs '
                        '(a file written with --tile); goes with --channels, not with --salvage, --partial or --recover; '
                        'measure: the metrics of this rectangle of both pictures, at least 16 pixels a side')
    p.add_argument('--min-psnr', dest='min_psnr', type=float, default=None, metavar='D',
                   help='compress / compress-dir: the smallest cap level (of the grid k C / 256) whose picture still reaches D dB against '
                        'the image; with --roi the rectangles stay uncapped and the level is the background\'s; prints the level, the '
                        'measure and the number of probes; transcode / transcode-dir: the smallest integer level 0 .. C whose picture '
                        'stays within D dB of the picture the file decodes to now; not with --cap, --max-bytes, --bpp or --background')
    p.add_argument('--min-ms-ssim', dest='min_ms_ssim', type=float, default=None, metavar='S', help='the same with an MS-SSIM of S in 0 .. 1')
    p.add_argument('--levels', type=int, default=None, metavar='N', help='rd: the N + 1 levels k C / N of the table, 1 <= N <= 256 (default 16)')
    p.add_argument('--rdo', type=float, default=None, metavar='LAMBDA',
                   help='compress / compress-dir: rate-aware symbol choice -- every symbol minimises distortion + LAMBDA * rate under the '
                        'context model, given the symbols before it (0: the quantiser\'s own symbols); any format, the file is read as '
                        'ever; goes with --cap / --roi / --background, not with --max-bytes, --bpp, --min-psnr or --min-ms-ssim; with '
                        '--depth expect a LARGER file: the choice moves fill symbols, which format 10 would have left uncoded')
    p.add_argument('--rdo-levels', dest='rdo_levels', default=None, metavar='a,b,..',
                   help='rd: rows over these lambdas of --rdo in place of cap levels; not with --levels or --roi')
    flags = p.parse_args(argv)
    from . import config_parser, val, weights as _weights
    try:
        ae_config, _ = config_parser.parse(_resolve_config(flags.ae_config, 'ae_configs', 'CONFIG_BASE_AE'))
        pc_config, _ = config_parser.parse(_resolve_config(flags.pc_config, 'pc_configs', 'CONFIG_BASE_PC'))
        if flags.command.endswith('-dir'):
            return _main_dir(flags, ae_config, pc_config)
        check_option_args(flags)
        layers = _layers_option(flags, ae_config.num_chan_bn)
        front_layers = _front_layers_option(flags, ae_config.num_chan_bn)
        if flags.weights == 'synthetic':
            wts = _weights.synthetic_weights(ae_config, pc_config, seed=flags.synthetic_seed)
        else:
            wts = val.load_weights_for_job(None, flags.weights, ae_config, pc_config)
        codec = Codec(ae_config, pc_config, wts, flags.device)
        if flags.command in ('compress', 'transcode', 'rd'):
            if flags.tile is not None:
                if flags.tile <= 0 or flags.tile % codec.factor != 0:
                    raise ValueError('--tile {} is not a positive multiple of the subsampling factor {}'.format(flags.tile, codec.factor))
                codec.tile = (flags.tile // codec.factor, flags.tile // codec.factor)
                codec.checked = flags.checked
                codec.order = 'wavefront' if flags.wavefront else 'raster'
                codec.layers = layers
                codec.front_layers = front_layers
                codec.depth_block = _depth_option(flags)
                codec.rans = _rans_option(flags)
            rois = [parse_roi_arg(r) for r in flags.roi or []]
        if flags.command == 'transcode':
            with open(flags.input, 'rb') as f:
                data = f.read()
            _transcode_one(flags, codec, flags.input, flags.output, data, rois=rois)
        elif flags.command == 'compress':
            if flags.max_bytes is not None or flags.bpp is not None:
                from PIL import Image
                img = np.asarray(Image.open(flags.input).convert('RGB'), dtype=np.uint8)     # as compress_file reads it
                data, level, probes = codec.compress_to_budget(img, _budget_of(flags, img.shape[0], img.shape[1]), rois=rois or None)
                with open(flags.output, 'wb') as f:
                    f.write(data)
                print(_compress_line(flags.output, data, img.shape[0] * img.shape[1]) + _budget_note(level, probes))
            elif _quality_of(flags) is not None:
                from PIL import Image
                img = np.asarray(Image.open(flags.input).convert('RGB'), dtype=np.uint8)     # as compress_file reads it
                data, level, m, probes = codec.compress_to_quality(img, rois=rois or None, **_quality_of(flags))
                with open(flags.output, 'wb') as f:
                    f.write(data)
                print(_compress_line(flags.output, data, img.shape[0] * img.shape[1]) + _quality_note(level, m, probes))
            elif flags.rdo is not None:
                from PIL import Image
                img = np.asarray(Image.open(flags.input).convert('RGB'), dtype=np.uint8)     # as compress_file reads it
                data, changed, count = codec.compress_counting(img, flags.rdo, cap=flags.cap, rois=rois or None, background=flags.background)
                with open(flags.output, 'wb') as f:
                    f.write(data)
                print(_compress_line(flags.output, data, img.shape[0] * img.shape[1]) + _rdo_note(flags.rdo, changed, count))
            elif flags.cap is not None or rois:
                data, pixels = codec.compress_file(flags.input, flags.output, cap=flags.cap, rois=rois or None, background=flags.background)
                print(_compress_line(flags.output, data, pixels))
            else:
                data, pixels = codec.compress_file(flags.input, flags.output)
                print(_compress_line(flags.output, data, pixels))
        elif flags.command == 'stream':
            _main_stream(flags, codec)
        elif flags.command == 'measure':
            from PIL import Image
            img = np.asarray(Image.open(flags.input).convert('RGB'), dtype=np.uint8)         # as compress_file reads it
            channels = check_channels(flags.channels, codec.C)
            rect = None if flags.region is None else parse_roi_arg(flags.region, '--region')
            with open(flags.output, 'rb') as f:
                data = f.read()
            m = codec.measure(img, data, channels=channels, rect=rect)
            print(_measure_line(flags.output, m, channels, codec.C, None if rect is None else _clip_rect(rect, img.shape[0], img.shape[1])))
        elif flags.command == 'rd':
            from PIL import Image
            img = np.asarray(Image.open(flags.input).convert('RGB'), dtype=np.uint8)         # as compress_file reads it
            key = 'level' if flags.rdo_levels is None else 'rdo'
            if flags.rdo_levels is not None:
                rows = codec.rdo_curve(img, parse_rdo_levels_arg(flags.rdo_levels))
            else:
                rows = codec.rd_curve(img, levels=rd_levels(codec.C, 16 if flags.levels is None else flags.levels), rois=rois or None)
            with open(flags.output, 'w') as f:
                json.dump(rd_table(codec, rows, flags.input, img.shape[0], img.shape[1], rois, key=key), f, indent=1)
                f.write('\n')
            for level, m in rows:
                print(_rd_line(level, m, 'lambda' if key == 'rdo' else key))
        elif flags.partial:
            from PIL import Image
            with open(flags.input, 'rb') as f:
                data = f.read()
            img, report = codec.decompress_partial(data)
            Image.fromarray(img).save(flags.output)
            print(_decompress_line(flags.output, img, len(data)))
            print(_partial_line(flags.input, report))
        elif getattr(flags, 'recover', False):
            from PIL import Image
            with open(flags.input, 'rb') as f:
                data = f.read()
            img, report = codec.recover(data)
            Image.fromarray(img).save(flags.output)
            print(_decompress_line(flags.output, img, len(data)))
            print(_recover_line(flags.input, report))
        elif flags.salvage:
            from PIL import Image
            with open(flags.input, 'rb') as f:
                data = f.read()
            try:
                img, report = codec.decompress(data), None
            except ValueError:
                img, report = codec.salvage(data)
            Image.fromarray(img).save(flags.output)
            print(_decompress_line(flags.output, img, len(data)))
            if report is not None and (report.damaged or not report.file_crc_ok):
                print(_damage_line(flags.input, report))
        elif getattr(flags, 'region', None) is not None:
            from PIL import Image
            channels = check_channels(flags.channels, codec.C)
            with open(flags.input, 'rb') as f:
                data = f.read()
            img = codec.decompress_region(data, parse_roi_arg(flags.region, '--region'), channels=channels)
            Image.fromarray(img).save(flags.output)
            print(_region_line(flags.output, img, codec.region_plan(parse_container(data), parse_roi_arg(flags.region, '--region')), channels, codec.C))
        else:
            channels = check_channels(flags.channels, codec.C)
            img = codec.decompress_file(flags.input, flags.output, channels=channels)
            print(_decompress_line(flags.output, img, os.path.getsize(flags.input), channels, codec.C))
    except ValueError as e:
        print('error: {}'.format(e), file=sys.stderr)
        return 2
    return 0


if __name__ == '__main__':
    sys.exit(main())

"""Image codec: an image to a self-describing file and back.

    python -m imgcomp_cvpr_amd.codec compress   IN.png  OUT.icf [--ae_config cvpr/low] [--pc_config cvpr/res_shallow] [--weights synthetic|FILE.npz|CKPT]
                                                                [--tile PIXELS]
    python -m imgcomp_cvpr_amd.codec decompress IN.icf  OUT.png [same options]

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
Every failure of parse / decompress is a ValueError that names the cause; nothing of a refused file reaches the device.
"""
import argparse
import io
import os
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


def tile_grid(h, w, th, tw):
    """the tiles of an (h, w) latent plane cut into th x tw blocks: [(y0, x0, th', tw')] in raster order, ceil(h / th) * ceil(w / tw)
    of them, the last row / column smaller where th / tw does not divide; every position is in exactly one tile."""
    h, w, th, tw = int(h), int(w), int(th), int(tw)
    if h < 1 or w < 1 or th < 1 or tw < 1:
        raise ValueError('tile grid: plane {} x {} and tile {} x {} must all be at least 1'.format(h, w, th, tw))
    return [(y0, x0, min(th, h - y0), min(tw, w - x0)) for y0 in range(0, h, th) for x0 in range(0, w, tw)]


def build_tiled_container(ae_name, pc_name, H, W, C, h, w, L, resolution, fingerprint, th, tw, first_syms, streams):
    """format 2: first_syms / streams per tile in the order of tile_grid(h, w, th, tw)."""
    a, p = ae_name.encode('utf-8'), pc_name.encode('utf-8')
    streams = [bytes(b) for b in streams]
    assert len(first_syms) == len(streams)
    head = b''.join([
        MAGIC, struct.pack('<H', FORMAT_VERSION_TILED),
        struct.pack('<H', len(a)), a, struct.pack('<H', len(p)), p,
        struct.pack('<II', H, W), struct.pack('<HII', C, h, w), struct.pack('<H', L),
        struct.pack('<d', float(resolution)), struct.pack('<I', fingerprint & 0xffffffff),
        struct.pack('<HH', th, tw), struct.pack('<I', len(streams))] +
        [struct.pack('<HI', f, len(b)) for f, b in zip(first_syms, streams)] +
        [struct.pack('<Q', sum(len(b) for b in streams))])
    body = head + b''.join(streams)
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
    """bytes -> Container (version 1) or TiledContainer (version 2).  Order: size, magic, version, CRC over the whole file -- only
    then are the header's lengths read, each against the bytes that remain; the payload length must equal exactly what is left
    before the CRC."""
    data = bytes(data)
    if len(data) < _MIN_SIZE:
        raise ValueError('truncated file: {} bytes, the smallest container has {}'.format(len(data), _MIN_SIZE))
    if data[:4] != MAGIC:
        raise ValueError('wrong magic {!r}: not a codec file (expected {!r})'.format(data[:4], MAGIC))
    version, = struct.unpack('<H', data[4:6])
    if version not in (FORMAT_VERSION, FORMAT_VERSION_TILED):
        raise ValueError('unsupported format version {} (this codec reads versions {} and {})'.format(
            version, FORMAT_VERSION, FORMAT_VERSION_TILED))
    stored, = struct.unpack('<I', data[-4:])
    actual = zlib.crc32(data[:-4]) & 0xffffffff
    if stored != actual:
        raise ValueError('CRC mismatch: file says {:08x}, content gives {:08x} (corrupt or truncated file)'.format(stored, actual))
    r = _Reader(data[:-4])
    r.take(6, 'magic and version')
    ae_name = r.take(r.unpack('<H', 'ae config name length')[0], 'ae config name')
    pc_name = r.take(r.unpack('<H', 'pc config name length')[0], 'pc config name')
    try:
        ae_name, pc_name = ae_name.decode('utf-8'), pc_name.decode('utf-8')
    except UnicodeDecodeError:
        raise ValueError('config name is not UTF-8')
    H, W = r.unpack('<II', 'image size')
    C, h, w = r.unpack('<HII', 'symbol volume shape')
    if version == FORMAT_VERSION_TILED:
        return _parse_tiled(r, version, ae_name, pc_name, H, W, C, h, w)
    L, first_sym = r.unpack('<HH', 'L and first symbol')
    resolution, = r.unpack('<d', 'frequency resolution')
    fingerprint, = r.unpack('<I', 'model fingerprint')
    n, = r.unpack('<Q', 'payload length')
    left = len(r.data) - r.pos
    if n != left:
        raise ValueError('payload length {} does not equal the {} bytes that remain in the file'.format(n, left))
    return Container(version, ae_name, pc_name, H, W, C, h, w, L, first_sym, resolution, fingerprint, r.take(n, 'payload'))


def _parse_tiled(r, version, ae_name, pc_name, H, W, C, h, w):
    """the rest of a format-2 file after the symbol volume shape (the CRC has been checked)."""
    L, = r.unpack('<H', 'L')
    resolution, = r.unpack('<d', 'frequency resolution')
    fingerprint, = r.unpack('<I', 'model fingerprint')
    th, tw = r.unpack('<HH', 'tile extent')
    ntiles, = r.unpack('<I', 'tile count')
    if th == 0 or tw == 0:
        raise ValueError('tile extent {} x {}: a tile has at least one row and one column'.format(th, tw))
    if h < 1 or w < 1:
        raise ValueError('symbol volume {} x {} cannot be tiled'.format(h, w))
    expected = ((h + th - 1) // th) * ((w + tw - 1) // tw)
    if ntiles != expected:
        raise ValueError('tile count {} does not equal the {} tiles of a {} x {} volume cut into {} x {}'.format(
            ntiles, expected, h, w, th, tw))
    table = r.take(6 * ntiles, 'tile table')              # against the bytes that remain, before anything of its size is built
    first_syms, lengths = [], []
    for t in range(ntiles):
        f, n_t = struct.unpack_from('<HI', table, 6 * t)
        if f >= L:
            raise ValueError('first symbol {} of tile {} is not below L = {}'.format(f, t, L))
        first_syms.append(f)
        lengths.append(n_t)
    n, = r.unpack('<Q', 'payload length')
    if sum(lengths) != n:
        raise ValueError('stream lengths of the {} tiles sum to {}, the payload length is {}'.format(ntiles, sum(lengths), n))
    left = len(r.data) - r.pos
    if n != left:
        raise ValueError('payload length {} does not equal the {} bytes that remain in the file'.format(n, left))
    payload = r.take(n, 'payload')
    streams, pos = [], 0
    for n_t in lengths:
        streams.append(payload[pos:pos + n_t])
        pos += n_t
    return TiledContainer(version, ae_name, pc_name, H, W, C, h, w, L, resolution, fingerprint, th, tw, first_syms, streams, payload)


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
    tile: None writes format 1; (th, tw) in symbol-volume units writes format 2, one stream per tile.  Reading needs no option:
    the file's version decides."""

    def __init__(self, ae_config, pc_config, weights, device='cuda', plan_flags=0, device_encode=True, tile=None):
        if tile is not None:
            tile = (int(tile[0]), int(tile[1]))
            if not (1 <= tile[0] <= 0xffff and 1 <= tile[1] <= 0xffff):
                raise ValueError('tile extent {} x {} is outside 1 .. 65535'.format(*tile))
        self.tile = tile
        import torch
        from . import autoencoder, probclass
        self.device = torch.device(device)
        self.ae = autoencoder.get_network_cls(ae_config)(ae_config).load_weights(weights, self.device)
        self.pc = probclass.get_network_cls(pc_config)(pc_config, num_centers=ae_config.num_centers).load_weights(weights, self.device)
        self.ae.plan_flags = int(plan_flags)
        self.pred = probclass.PredictionNetwork(self.pc, pc_config, self.ae.get_centers_variable())
        self.ae_name, self.pc_name = config_name(ae_config), config_name(pc_config)
        self.factor = int(self.ae.get_subsampling_factor())
        self.C, self.L = int(ae_config.num_chan_bn), int(ae_config.num_centers)
        self.device_encode = bool(device_encode)
        self.fingerprint = model_fingerprint(self.ae.get_centers_variable().detach().cpu().numpy(),
                                             {n: t.detach().cpu().numpy() for n, t in self.pc._params.items()})

    # -- the two halves, also usable on their own (tests compare their intermediate values) --

    def encode_symbols(self, img_hwc_uint8):
        """HWC uint8 -> (EncoderOutput of the padded image, (H, W))."""
        import torch
        from . import val
        img = np.asarray(img_hwc_uint8)
        if img.ndim != 3 or img.shape[2] not in (3, 4) or img.dtype != np.uint8:
            raise ValueError('expected an HWC uint8 image with 3 channels, got {} {}'.format(img.shape, img.dtype))
        img = img[:, :, :3]
        H, W = int(img.shape[0]), int(img.shape[1])
        padded, _ = val.add_padding(img, self.factor)
        x = torch.as_tensor(np.ascontiguousarray(np.transpose(padded, (2, 0, 1)))[None]).to(self.device).float()
        return self.ae.encode(x, is_training=False), (H, W)

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

    def compress(self, img_hwc_uint8):
        enc, (H, W) = self.encode_symbols(img_hwc_uint8)
        sym = enc.symbols[0]
        C, h, w = (int(v) for v in sym.shape)
        if self.tile is not None:
            th, tw = self.tile
            coded = self.pred.encode_tiles(sym, th, tw)
            return build_tiled_container(self.ae_name, self.pc_name, H, W, C, h, w, self.L, self.pred.freqs_resolution,
                                         self.fingerprint, th, tw, [f for _, f in coded], [b for b, _ in coded])
        if self.device_encode:
            payload, first_sym = self.pred.encode_stream(sym)
        else:
            payload, first_sym = self._host_encode_stream(sym.cpu().numpy())
        return build_container(self.ae_name, self.pc_name, H, W, C, h, w, self.L, first_sym, self.pred.freqs_resolution,
                               self.fingerprint, payload)

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
        for first_sym in (c.first_syms if isinstance(c, TiledContainer) else [c.first_sym]):
            if first_sym >= c.L:
                raise ValueError('header mismatch: first symbol {} is not below L = {}'.format(first_sym, c.L))
        if c.resolution != self.pred.freqs_resolution:
            raise ValueError('header mismatch: frequency resolution {} in the file, {} in the model'.format(
                c.resolution, self.pred.freqs_resolution))

    def decode_symbols(self, data):
        """container bytes of either format -> (symbols (C,h,w) int64 numpy, Container or TiledContainer)."""
        c = parse_container(data)
        self.check_container(c)
        try:
            if isinstance(c, TiledContainer):
                sym = self.pred.decode_tiles(c.streams, c.first_syms, (c.C, c.h, c.w), c.th, c.tw)
            else:
                sym = self.pred.decode_stream(c.payload, (c.C, c.h, c.w), c.first_sym)
        except ValueError as e:
            raise ValueError('decoder status is not 0: {}'.format(e))
        return sym, c

    def decompress(self, data):
        import torch
        sym, c = self.decode_symbols(data)
        s = torch.as_tensor(sym).to(self.device)
        q = self.ae.get_centers_variable()[s][None].contiguous()
        x_out = self.ae.decode(q, is_training=False).to(torch.uint8)            # tf.cast truncates (val.py)
        img = np.transpose(x_out[0].cpu().numpy(), (1, 2, 0))
        f = self.factor
        t, l = ((-c.H) % f) // 2, ((-c.W) % f) // 2                               # val.add_padding's offsets
        return np.ascontiguousarray(img[t:t + c.H, l:l + c.W, :])

    def compress_file(self, image_path, out_path):
        from PIL import Image
        img = np.asarray(Image.open(image_path).convert('RGB'), dtype=np.uint8)     # as val.load_image_chw reads it
        data = self.compress(img)
        with open(out_path, 'wb') as f:
            f.write(data)
        return data, img.shape[0] * img.shape[1]

    def decompress_file(self, in_path, image_path):
        from PIL import Image
        with open(in_path, 'rb') as f:
            data = f.read()
        img = self.decompress(data)
        Image.fromarray(img).save(image_path)
        return img


def _resolve_config(arg, tree, env):
    from . import config_parser
    if os.path.isfile(arg):
        return arg
    base = os.environ.get(env, config_parser.builtin_config_path(tree))
    p = os.path.join(base, *arg.split('/'))
    if not os.path.isfile(p):
        raise ValueError('config {!r} not found (a file, or a name below {})'.format(arg, base))
    return p


def main(argv=None):
    p = argparse.ArgumentParser(description='compress an image to a codec file, or a codec file back to an image')
    p.add_argument('command', choices=['compress', 'decompress'])
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
    flags = p.parse_args(argv)
    from . import config_parser, val, weights as _weights
    try:
        ae_config, _ = config_parser.parse(_resolve_config(flags.ae_config, 'ae_configs', 'CONFIG_BASE_AE'))
        pc_config, _ = config_parser.parse(_resolve_config(flags.pc_config, 'pc_configs', 'CONFIG_BASE_PC'))
        if flags.weights == 'synthetic':
            wts = _weights.synthetic_weights(ae_config, pc_config, seed=flags.synthetic_seed)
        else:
            wts = val.load_weights_for_job(None, flags.weights, ae_config, pc_config)
        codec = Codec(ae_config, pc_config, wts, flags.device)
        if flags.command == 'compress':
            if flags.tile is not None:
                if flags.tile <= 0 or flags.tile % codec.factor != 0:
                    raise ValueError('--tile {} is not a positive multiple of the subsampling factor {}'.format(flags.tile, codec.factor))
                codec.tile = (flags.tile // codec.factor, flags.tile // codec.factor)
            data, pixels = codec.compress_file(flags.input, flags.output)
            c = parse_container(data)
            payload = len(c.payload)
            tiles = ', {} tiles'.format(len(c.streams)) if isinstance(c, TiledContainer) else ''
            print('{}: {} bytes, payload {} bytes = {:.4f} bpp, file {:.4f} bpp{}'.format(
                flags.output, len(data), payload, 8.0 * payload / pixels, 8.0 * len(data) / pixels, tiles))
        else:
            img = codec.decompress_file(flags.input, flags.output)
            size = os.path.getsize(flags.input)
            print('{}: {} x {} from {} bytes = {:.4f} bpp'.format(flags.output, img.shape[0], img.shape[1], size,
                                                                 8.0 * size / (img.shape[0] * img.shape[1])))
    except ValueError as e:
        print('error: {}'.format(e), file=sys.stderr)
        return 2
    return 0


if __name__ == '__main__':
    sys.exit(main())

#!/usr/bin/env python3
"""Watch the interactive form from a browser: an MJPEG stream (multipart/x-mixed-replace) of a present_jpeg loop
(fspt_present_jpeg) over the built-in scene, or over --scene.  Frames are drawn and JPEG-encoded on the GPU;
a frame is a few hundred KB on the wire.  Standard library only; binds to 127.0.0.1 (forward the port to look from elsewhere).
    usage: python tools/view_server.py [--port 8080] [--width 960] [--height 540] [--scene web/scene/bunny.json] [--quality 85]
    then open http://127.0.0.1:8080/ (the page) or /stream (the stream itself)"""
import argparse
import http.server
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOUNDARY = "fsptframe"
PAGE = b"<!doctype html><title>fspt</title><body style='margin:0;background:#111'><img src='/stream' style='max-width:100%'>"


def mjpeg_part(jpeg_bytes):
    """One part of the multipart/x-mixed-replace body: the boundary line, the part's headers, the file, CRLF"""
    head = f"--{BOUNDARY}\r\nContent-Type: image/jpeg\r\nContent-Length: {len(jpeg_bytes)}\r\n\r\n"
    return head.encode("ascii") + bytes(jpeg_bytes) + b"\r\n"


def make_tracer(a):
    import fspt_amd
    from fspt_amd import scene as S
    if a.scene:
        from fspt_amd import scene_file as F
        arrays, settings = F.load_scene_file(a.scene, a.assets)
        pt = fspt_amd.PathTracer(arrays, a.width, a.height, num_bounces=a.bounces)
        pt.eye, pt.dir = list(settings["eye"]), list(settings["dir"])  # (the scene file's view, as scene_file.render_frame sets it)
        pt.fovScale, pt.envTheta = settings["fov_scale"], settings["env_theta"]
        pt.lensFeatures = [settings["focus"], settings["aperture"]]
        return pt, float(settings["exposure"])
    pt = fspt_amd.PathTracer(S.bunny_scene(n=a.mesh_n), a.width, a.height, num_bounces=a.bounces)
    pt.set_camera(**S.BUNNY_CAMERA)
    return pt, 1.0


def frames(pt, exposure, quality, s444, max_ticks):
    """The files of a present_jpeg loop: one tick per frame while the picture still converges, then the same frame again"""
    while True:
        if pt.pingpong < max_ticks:
            pt.tick()
        data, ticks = pt.present_jpeg(exposure=exposure, quality=quality, subsampling="444" if s444 else "420")
        if ticks:
            yield data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--port", type=int, default=8080)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--mesh-n", type=int, default=76)
    ap.add_argument("--scene", default=None)
    ap.add_argument("--assets", default=None)
    ap.add_argument("--quality", type=int, default=85)
    ap.add_argument("--444", dest="s444", action="store_true")
    ap.add_argument("--max-ticks", type=int, default=4096, help="stop adding samples after this many ticks")
    a = ap.parse_args()
    pt, exposure = make_tracer(a)

    class Handler(http.server.BaseHTTPRequestHandler):
        def do_GET(self):
            if self.path != "/stream":
                self.send_response(200)
                self.send_header("Content-Type", "text/html")
                self.send_header("Content-Length", str(len(PAGE)))
                self.end_headers()
                self.wfile.write(PAGE)
                return
            self.send_response(200)
            self.send_header("Content-Type", f"multipart/x-mixed-replace; boundary={BOUNDARY}")
            self.send_header("Cache-Control", "no-store")
            self.end_headers()
            pt.clear()  # a new viewer watches the picture converge from its first sample
            try:
                for data in frames(pt, exposure, a.quality, a.s444, a.max_ticks):
                    self.wfile.write(mjpeg_part(data))
            except (BrokenPipeError, ConnectionResetError):
                pass

    # one viewer at a time: all calls for one target come from one thread (include/fspt.h)
    srv = http.server.HTTPServer(("127.0.0.1", a.port), Handler)
    print(f"serving http://127.0.0.1:{a.port}/  ({a.width}x{a.height}, quality {a.quality})", flush=True)
    try:
        srv.serve_forever()
    except KeyboardInterrupt:
        pass
    finally:
        pt.close()


if __name__ == "__main__":
    main()

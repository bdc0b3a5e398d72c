"""Front door aggregate frames/s with N interleaved 640x480 gray cameras on one connection against one camera (GPU box).

The process plays the host (one TCP connection, u32 length + MessagePack map per frame, PGM payload) the way bench.py's
front door leg does: calibrations of every camera, then 192 pre-encoded frames sent with one sendall, camera k's frames
of its own parallax sequence (back and forth), round-robin over the cameras; a "features" message per frame says when it
has been answered.  Rate = frames answered after the first read-ahead batch / time from that batch's last answer to the
last answer.  Read-ahead 16 (SENDSLAM_NO_PACING=1), 1250 features.
usage: python profiles/tools/frontdoor_multicam.py [n_cameras ...]   (default: 1 4)"""
import os
import socket
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "send-slam_amd"))
import msgpack  # noqa: E402

from send_slam_amd import synth, wire  # noqa: E402

W, H, N_FRAMES, READAHEAD, N_DISTINCT = 640, 480, 192, 16, 24


def run(n_cams):
    dims = {"width": W, "height": H, "channels": 1}
    enc = {}
    for c in range(1, n_cams + 1):
        sc = synth.scene(4000 + c, W, H)
        enc[c] = [wire.encode_to_ppm(synth.parallax_frame(4000 + c, W, H, t, sc=sc)) for t in range(N_DISTINCT)]
    order = list(range(N_DISTINCT)) + list(range(N_DISTINCT - 2, 0, -1))  # back and forth: continuous motion
    pk, t_of = [], {}
    for i in range(N_FRAMES):
        c = 1 + i % n_cams
        t_of[c] = t_of.get(c, -1) + 1
        pk.append(wire.build_frame_packet(enc[c][order[t_of[c] % len(order)]], dims, camera_id=c, timestamp=1.0 + t_of[c] / 30.0))
    calib = b"".join(wire.build_calibration_packet([[0.8 * W, 0, W / 2], [0, 0.8 * W, H / 2], [0, 0, 1]], [0, 0, 0, 0], dims, camera_id=c)
                     for c in range(1, n_cams + 1))
    srv = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
    srv.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
    srv.bind(("127.0.0.1", 0))
    srv.listen(1)
    env = dict(os.environ, ORB_SLAM3_WS_PORT=str(srv.getsockname()[1]), SENDSLAM_NO_PACING="1", SENDSLAM_READAHEAD=str(READAHEAD),
               SENDSLAM_EMIT_FEATURES="1", LD_LIBRARY_PATH=os.path.join(ROOT, "send-slam_amd", "lib") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    proc = subprocess.Popen([os.path.join(ROOT, "send-slam_amd", "frontdoor", "sendslam_frontdoor")], env=env, stdout=subprocess.PIPE,
                            stderr=subprocess.STDOUT, text=True)
    stamps, states = [], []
    try:
        srv.settimeout(60)
        conn, _ = srv.accept()
        conn.settimeout(120)
        conn.setsockopt(socket.SOL_SOCKET, socket.SO_SNDBUF, 8 << 20)

        def reader():
            buf = b""
            while len(stamps) < N_FRAMES:
                chunk = conn.recv(1 << 16)
                if not chunk:
                    return
                pkts, buf = wire.extract_packets(buf + chunk)
                for p_ in pkts:
                    m = msgpack.unpackb(p_, raw=False)
                    if m.get("type") == "features":
                        stamps.append(time.perf_counter())
                        states.append(m["tracking_state"])
        conn.sendall(calib)
        th = threading.Thread(target=reader)
        th.start()
        conn.sendall(b"".join(pk))
        th.join(timeout=180)
        conn.sendall(wire.build_terminate_packet())
        log = proc.communicate(timeout=60)[0]
    finally:
        srv.close()
        if proc.poll() is None:
            proc.kill()
    if len(stamps) < N_FRAMES:
        return {"error": f"{len(stamps)} of {N_FRAMES} frames answered", "log_tail": log[-400:]}
    rate = (N_FRAMES - READAHEAD) / (stamps[-1] - stamps[READAHEAD - 1])
    return {"cameras": n_cams, "frames_per_s": round(rate, 1), "frames_tracking_ok": states.count(2), "frames": N_FRAMES}


if __name__ == "__main__":
    for n in [int(a) for a in sys.argv[1:]] or [1, 4]:
        print(run(n), flush=True)

// A MONO8 camera frame through cv::linemod::Detector::match without the node's mixChannels (include/lmx_cv_linemod.hpp, gray contexts):
// the same detector is handed the CV_8UC1 frame and the frame copied into B, G and R -- alternating, the way a node that serves both kinds of
// camera would call it -- and prints every call's matches.  tests/test_gpu_gray.py checks that all calls agree and equal the oracle.
//
// usage: cv_gray_main <templates.yml> <W> <H> <frame_cols> <crop_x> <threshold> <gray.raw> [depth.raw]
#include <opencv2/opencv.hpp>          // the stand-in under tests/cpp/cv_standin (a real build has OpenCV here)
#include "lmx_cv_linemod.hpp"

#include <cstdio>
#include <fstream>
#include <iostream>

using namespace cv;
using namespace std;

static std::vector<char> slurp(const char* p) {
  std::ifstream f(p, std::ios::binary);
  return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
  if (argc < 8) return 2;
  const int W = atoi(argv[2]), H = atoi(argv[3]), frame_cols = atoi(argv[4]), crop_x = atoi(argv[5]);
  const float threshold = (float)atof(argv[6]);
  std::vector<char> gray = slurp(argv[7]), depth;
  if ((int)gray.size() != H * frame_cols) { fprintf(stderr, "gray.raw: %zu bytes\n", gray.size()); return 1; }
  if (argc > 8) depth = slurp(argv[8]);
  std::vector<char> bgr((size_t)H * W * 3);   // what the node's mixChannels made of the crop
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x)
      for (int c = 0; c < 3; ++c) bgr[((size_t)y * W + x) * 3 + c] = gray[(size_t)y * frame_cols + crop_x + x];
  try {
    cv::linemod::Detector detector;
    cv::FileStorage fs(argv[1], cv::FileStorage::READ);
    if (!fs.isOpened()) { fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
    detector.read(fs.root());
    cv::FileNode fn = fs["classes"];
    for (cv::FileNodeIterator i = fn.begin(), iend = fn.end(); i != iend; ++i) detector.readClass(*i);
    Mat gframe(H, frame_cols, CV_8UC1, gray.data());
    Mat bframe(H, W, CV_8UC3, bgr.data());
    Mat dframe;
    if (!depth.empty()) dframe = Mat(H, frame_cols, CV_16UC1, depth.data());
    const char* kinds[4] = {"gray", "bgr", "gray", "bgr"};
    for (int call = 0; call < 4; ++call) {
      std::vector<Mat> sources;
      if (call % 2 == 0) sources.push_back(gframe(Rect(crop_x, 0, W, H)));   // ROI view of the MONO8 frame: row stride frame_cols bytes
      else sources.push_back(bframe);
      if (!dframe.empty()) sources.push_back(dframe(Rect(crop_x, 0, W, H)));
      std::vector<linemod::Match> matches;
      std::vector<Mat> quantized;
      detector.match(sources, threshold, matches, std::vector<String>(), quantized);
      unsigned long qsum = 0;
      for (size_t k = 0; k < quantized.size(); ++k)
        for (int i = 0; i < quantized[k].rows * quantized[k].cols; ++i) qsum = qsum * 31 + quantized[k].data[i];
      printf("call %d %s matches %zu quantized %zu %lu\n", call, kinds[call], matches.size(), quantized.size(), qsum);
      for (size_t i = 0; i < matches.size(); ++i)
        printf("%d %d %.9g %d %s\n", matches[i].x, matches[i].y, matches[i].similarity, matches[i].template_id, matches[i].class_id.c_str());
    }
  } catch (const std::exception& e) {
    fprintf(stderr, "exception %s\n", e.what());
    return 1;
  }
  return 0;
}

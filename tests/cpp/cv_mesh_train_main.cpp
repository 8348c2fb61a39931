// The cv::linemod-shaped facade (include/lmx_cv_linemod.hpp) training a bank from a mesh: Detector(modalities, T) as the reference's
// trainer builds it (src/renderer.cpp:179-185), Detector::addTemplatesFromMesh in place of its render + addTemplate loop, writeLinemod as
// src/renderer.cpp:56-70.  Built against the stand-in OpenCV core types by tests/test_gpu_mesh_train.py.
//   cv_mesh_train_main <triangles.f64> <views.f64> <width> <height> <focal> <out_templates.yml>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include <opencv2/opencv.hpp>
#include "lmx_cv_linemod.hpp"

static std::vector<double> read_doubles(const char* path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) { std::fprintf(stderr, "cannot open %s\n", path); std::exit(1); }
  std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<double> out(raw.size() / sizeof(double));
  std::memcpy(out.data(), raw.data(), out.size() * sizeof(double));
  return out;
}

static void writeLinemod(const cv::Ptr<cv::linemod::Detector>& detector, const std::string& filename) {
  cv::FileStorage fs(filename, cv::FileStorage::WRITE);
  detector->write(fs);
  std::vector<cv::String> ids = detector->classIds();
  fs << "classes" << "[";
  for (int i = 0; i < (int)ids.size(); ++i) {
    fs << "{";
    detector->writeClass(ids[i], fs);
    fs << "}";
  }
  fs << "]";
}

int main(int argc, char** argv) {
  if (argc != 7) { std::fprintf(stderr, "usage: cv_mesh_train_main triangles.f64 views.f64 width height focal out.yml\n"); return 2; }
  try {
    const std::vector<double> tri = read_doubles(argv[1]), vw = read_doubles(argv[2]);
    std::vector<lmx_mesh_view> views(vw.size() / 10);
    std::memcpy(views.data(), vw.data(), views.size() * sizeof(lmx_mesh_view));
    lmx_mesh_camera cam;
    cam.width = std::atoi(argv[3]); cam.height = std::atoi(argv[4]);
    cam.fx = cam.fy = std::atof(argv[5]);
    cam.cx = cam.width / 2.0; cam.cy = cam.height / 2.0;
    cam.light[0] = 0.35; cam.light[1] = -0.45; cam.light[2] = -0.82;
    std::vector<cv::Ptr<cv::linemod::Modality> > modalities;
    modalities.push_back(cv::Ptr<cv::linemod::ColorGradient>(new cv::linemod::ColorGradient));
    modalities.push_back(cv::Ptr<cv::linemod::DepthNormal>(new cv::linemod::DepthNormal));
    std::vector<int> T;
    T.push_back(5);
    T.push_back(8);
    cv::Ptr<cv::linemod::Detector> detector_(new cv::linemod::Detector(modalities, T));
    const std::vector<int> ids = detector_->addTemplatesFromMesh(tri, cam, views, "obj");
    int accepted = 0;
    for (size_t i = 0; i < ids.size(); ++i) accepted += ids[i] >= 0;
    std::printf("views %d accepted %d templates %d\n", (int)ids.size(), accepted, detector_->numTemplates());
    writeLinemod(detector_, argv[6]);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 1;
  }
  return 0;
}

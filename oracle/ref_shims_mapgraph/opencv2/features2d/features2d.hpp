// Stand-in for <opencv2/features2d/features2d.hpp> in the map-graph build: Tracking.h and Tracking.cc include it and use nothing of it
// beyond cv::KeyPoint, which the core stand-in declares.
#pragma once
#include <opencv2/core/core.hpp>
